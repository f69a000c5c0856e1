/*
 * pioneer_amd.h — C ABI of the MI355X-native Pioneer-arm step/rollout engine.
 *
 * The reference (xdralex/pioneer) has no FFI layer: its boundary is the Python
 * gym.Env protocol of pioneer/envs/pioneer/pioneer_knm_env.py as consumed by
 * RLlib.  This header is the C-ABI a maintainer would bind in place of that
 * Python hot path; every entry point names the reference interface it
 * replaces (file:line, relative to the reference tree).
 *
 * Conventions
 *   - every function returns an int status (PNR_OK == 0, < 0 on error); no
 *     exceptions cross the boundary; pnr_last_error() gives the message;
 *   - all I/O buffers are caller-owned DEVICE pointers (plain pointers and
 *     sizes; no torch types); the library owns only the per-env state;
 *   - calls are asynchronous on the given HIP stream (passed as void*, i.e.
 *     a hipStream_t; NULL = the default stream) and never synchronise — with
 *     ONE exception: pnr_create zero-fills the state planes on the NULL stream
 *     and waits for that fill (hipStreamSynchronize(NULL)) before it returns,
 *     so that a first pnr_reset on ANY stream, blocking or not, finds them
 *     zero (pnr_destroy frees memory and synchronises as hipFree does);
 *     and a SECOND, of the same kind: the first pnr_set_body_params of a
 *     handle allocates the sphere buffer, zero-fills it on the NULL stream
 *     and waits for that fill, so that every env is inert on every stream;
 *   - a handle is not thread-safe; distinct handles are independent;
 *   - there is NO CPU backend: pnr_create fails with PNR_ERR_NODEVICE when no
 *     gfx950 device is usable.
 */
#ifndef PIONEER_AMD_H
#define PIONEER_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an exported signature or struct changes incompatibly; a caller checks pnr_abi_version() == the
 * PNR_ABI_VERSION it was compiled against before any other call (pnr_config carries it too).
 *   1  round 1
 *   2  pnr_ppo_loss gained `idx` (argument 2) and `means` (before `stream`); pnr_config grew (guarded by struct_size)
 *   3  pnr_mlp_step gained first_net / n_nets (the two nets as two chains) and w3_partials / w3_partial_floats (layer 3's
 *      weight-gradient partials made by the fused kernel); new entry points pnr_ppo_rollout (the sampler's T steps as one
 *      resident launch), pnr_filter_prepare, pnr_mlp_w3_partial_floats
 *   4  float32-accurate operands for the MLP kernels: pnr_mlp_pack / pnr_mlp_forward / pnr_mlp_act / pnr_mlp_gather gained `planes`
 *      (before `stream`), pnr_mlp_step gained `planes`; pnr_create waits for its zero fill (Conventions)
 *   5  new entry points pnr_world_step, pnr_set_joint_motor, pnr_build_fingerprint; `planes` == 2 now means two SCALED FP16 planes
 *      (was: two bf16 planes) in every pnr_mlp_* call; pnr_mlp_train_step checks every argument before its first launch and
 *      accepts g_head == NULL with w3_partials; later, additively: pnr_get_link_states, pnr_render,
 *      pnr_get_jacobian, pnr_ik_params_default, pnr_solve_ik, pnr_inverse_dynamics, pnr_mass_matrix, pnr_world_step_torques,
 *      pnr_contact_params_default, pnr_get_contacts, pnr_ik_pose_params_default, pnr_solve_ik_pose, pnr_ray_params_default,
 *      pnr_ray_test, pnr_world_step_wrenches, pnr_get_joint_states, pnr_world_step_targets, pnr_body_params_default,
 *      pnr_set_body_params, pnr_set_body_state, pnr_get_body_state, pnr_render_bodies, pnr_set_body_queries,
 *      pnr_render_cameras, pnr_body_grip_params_default, pnr_set_body_grip_params, pnr_set_body_grip, pnr_get_body_grip,
 *      pnr_ik_multi_params_default, pnr_solve_ik_multi, pnr_path_params_default, pnr_path_clearance,
 *      pnr_ik_path_params_default, pnr_solve_ik_path, pnr_retime_params_default, pnr_retime_workspace_bytes, pnr_retime_path,
 *      pnr_traj_sample_params_default, pnr_sample_trajectory */
#define PNR_ABI_VERSION 5

#define PNR_DOF 6          /* revolute joints of pioneer_knm_6dof.urdf:209-264 */
#define PNR_OBS_DIM 137    /* pioneer_knm_env.py:194-211 (26 pieces)         */
#define PNR_STATE_WORDS 24 /* a[6] v[6] r[6] target[3] potential step episode */
#define PNR_INFO_DIM 4     /* r_pot, r_step, r_done, dist (numeric subset of   */
                           /* the info dict, pioneer_knm_env.py:167-179)      */
#define PNR_DYN_STATE_WORDS 36 /* dynamics mode: q[6] qd[6] + 24 params       */
#define PNR_BODY_STATE_WORDS 8 /* the moving sphere: position[3] velocity[3] mass radius */
#define PNR_BODY_GRIP_WORDS 4  /* the grip on the moving sphere: max_force, last force on the sphere[3] */
#define PNR_NUM_LINKS 11       /* pnr_get_link_states: links per env (URDF joint order) */
#define PNR_LINK_STATE_DIM 13  /* floats per link record                      */
#define PNR_JACOBIAN_DIM 36    /* pnr_get_jacobian: 6 rows x 6 joint columns per env */

enum pnr_status {
    PNR_OK = 0,
    PNR_ERR_INVALID = -1,     /* bad argument (AssertionError in the reference) */
    PNR_ERR_HIP = -2,         /* a HIP runtime call failed                      */
    PNR_ERR_NOMEM = -3,
    PNR_ERR_NODEVICE = -4,    /* no usable gfx950 device                        */
    PNR_ERR_UNSUPPORTED = -5
};

/* Memory layout of a [num_envs x F] batch. */
enum pnr_layout {
    PNR_ENV_MAJOR = 0,     /* row-major [num_envs][F] — what gym/RLlib see      */
    PNR_FEATURE_MAJOR = 1  /* [F][num_envs] — feature planes (first Linear as W . X^T)      */
};

/* The reference's motor forms (Joint.control_position / control_velocity, bullet_scene.py:123-155).  0 and 1 are the engine's PD
 * torque law (pnr_config.control_mode and pnr_set_joint_motor); 2 and 3 are Bullet's velocity-level constraint motor, accepted by
 * pnr_set_joint_motor only (pnr_create rejects them: the step's law is the PD law). */
enum pnr_control {
    PNR_CONTROL_POSITION = 0, /* POSITION_CONTROL: positionGain pd_kp, velocityGain pd_kd, force torque_limit, maxVelocity */
    PNR_CONTROL_VELOCITY = 1, /* VELOCITY_CONTROL: the motor tracks the commanded velocity only (gain pd_kd, force torque_limit) */
    PNR_CONTROL_POSITION_CONSTRAINT = 2, /* Bullet's POSITION_CONTROL motor: a constraint on the joint velocity (pnr_set_joint_motor) */
    PNR_CONTROL_VELOCITY_CONSTRAINT = 3  /* Bullet's VELOCITY_CONTROL motor: a constraint on the joint velocity (pnr_set_joint_motor) */
};

/* Bullet's values for the arguments of a constraint motor (PNR_CONTROL_*_CONSTRAINT) that the caller leaves out (NaN).  RECALLED
 * from pybullet's setJointMotorControl2 and btMultiBodyJointMotor, NOT verified against Bullet. */
#define PNR_BULLET_POSITION_GAIN 0.1        /* positionGain (recalled, not verified) */
#define PNR_BULLET_VELOCITY_GAIN 1.0        /* velocityGain (recalled, not verified) */
#define PNR_BULLET_TARGET_VELOCITY 0.0      /* targetVelocity (recalled, not verified) */
#define PNR_BULLET_MAX_FORCE 100000.0       /* force: pybullet's setJointMotorControl2 default (recalled, not verified) */
#define PNR_BULLET_MAX_VELOCITY 0.0         /* maxVelocity: none (pybullet's -1; recalled, not verified) */

enum pnr_mode {
    PNR_MODE_KINEMATIC = 0, /* the reference's live semantics ("parity mode")   */
    PNR_MODE_DYNAMIC = 1    /* ABA forward dynamics + PD torque tracking         */
};

/*
 * A static body of the scene: what World/Scene.create_body_plane / create_body_box / create_body_sphere make with mass 0
 * and a collision shape (bullet_scene.py:193-246).  Dynamics mode only: every contact sample sphere of the arm (the
 * pointer; with link_contacts the 22 link samples too) collides with it, surface to surface, by the penalty law of
 * contact_kp / contact_kd.  orientation is Bullet's quaternion (x, y, z, w).
 */
#define PNR_MAX_SCENE 8
enum pnr_shape { PNR_SHAPE_NONE = 0, PNR_SHAPE_PLANE = 1, PNR_SHAPE_BOX = 2, PNR_SHAPE_SPHERE = 3 };
typedef struct pnr_scene_body {
    int32_t shape;                /* enum pnr_shape */
    int32_t reserved;
    double position[3];           /* basePosition */
    double orientation[4];        /* baseOrientation (x, y, z, w) */
    double size[3];               /* plane: planeNormal in the body frame; box: halfExtents; sphere: radius in size[0] */
} pnr_scene_body;

/*
 * Tunables.  Field names and defaults follow PioneerKinematicConfig
 * (pioneer_knm_env.py:19-34) and SimulationConfig (bullet_env.py:36-44);
 * max_episode_steps is gym.wrappers.TimeLimit's argument
 * (pioneer/launch/pioneer_knm_train.py:27).  Fill with pnr_config_default().
 */
typedef struct pnr_config {
    uint32_t struct_size; /* sizeof(pnr_config), checked by pnr_create */
    uint32_t abi_version; /* PNR_ABI_VERSION */

    /* PioneerKinematicConfig */
    double max_v_to_r;            /* 2       */
    double max_a_to_v;            /* 10      */
    double done_distance;         /* 0.1     */
    double award_max;             /* 100.0   */
    double award_done;            /* 5.0     */
    double award_potential_slope; /* 10.0    */
    double penalty_step;          /* 1/100   */
    double target_lo[3];          /* (15,-10,2) */
    double target_hi[3];          /* (25, 10,6) */
    double target_radius;         /* 0.2 (visual only in the reference) */

    /* SimulationConfig */
    double timestep;              /* 1/240 */
    int32_t frame_skip;           /* 10    */
    double gravity;               /* 0     */

    /* TimeLimit; 0 disables truncation */
    int32_t max_episode_steps;    /* 500   */

    /* engine options (no reference counterpart) */
    int32_t auto_reset;           /* 1: done|truncated envs are re-drawn in-kernel */
    int32_t obs_layout;           /* enum pnr_layout */
    int32_t action_layout;        /* enum pnr_layout */
    int32_t mode;                 /* enum pnr_mode */

    /* dynamics mode only (PD surface of bullet_scene.py:123-155; unpinned) */
    double pd_kp;                 /* position gain  [torque/rad]         */
    double pd_kd;                 /* velocity gain  [torque/(rad/s)]     */
    double torque_limit;          /* |tau| cap; <= 0 = unlimited         */
    double joint_damping;         /* viscous, URDF default 0             */
    double joint_friction;        /* Coulomb (smoothed), URDF default 0  */
    int32_t teleport;             /* 1: reference semantics — q:=r, qd:=0 before the sub-steps */
    int32_t randomize;            /* 1: per-env link-mass / friction / damping draws at reset  */
    double rand_mass_lo, rand_mass_hi;         /* scale on every link mass, U(lo,hi) */
    double rand_friction_lo, rand_friction_hi; /* per-joint Coulomb friction         */
    double rand_damping_lo, rand_damping_hi;   /* per-joint viscous damping          */
    double ground_z;              /* contact plane height for the pointer; NaN = no plane */
    double contact_kp, contact_kd;/* penalty contact stiffness / damping  */
    /* static box obstacle for the pointer sphere (the reference demo's create_body_box,
     * pioneer_knm_env.py:249-255: half extents (0.5,0.5,5) at (10,5,0)); half extent <= 0 = none */
    double obstacle_position[3];
    double obstacle_half_extents[3];
    double pointer_radius;        /* 0.2: the pointer's sphere (urdf:190-196) */
    int32_t control_mode;         /* enum pnr_control; dynamics mode, teleport 0 */
    int32_t link_contacts;        /* 1: sample spheres along every moving link collide with the plane / box too (capsules
                                   * fitted to the URDF's visual boxes; the URDF itself has no <collision>) */
    double max_velocity;          /* control_position's maxVelocity (bullet_scene.py:126,136): cap on the velocity the
                                   * motor asks for, rad/s; <= 0 = none */
    int32_t n_scene;              /* static scene bodies in use, 0 .. PNR_MAX_SCENE */
    int32_t pd_inertia_scaled;    /* 1: the motor asks for an ACCELERATION pd_kp (r - q) + pd_kd (v* - qd) and applies the torque
                                   * clip(D_i x that, +-torque_limit), D_i being joint i's articulated-body inertia at the current
                                   * pose (the ABA forms it anyway): pd_kp = omega^2 and pd_kd = 2 zeta omega then hold for every
                                   * joint and pose alike, and the explicit motor is stable whenever pd_kd x timestep < 2 — on the
                                   * light wrist (inertia 6.6) as on the shoulder (1477).  Bullet's own motors are implicit
                                   * constraints and need no such care.  0: plain torque gains, the same for all joints */
    pnr_scene_body scene[PNR_MAX_SCENE];
} pnr_config;

typedef struct pnr_env_s* pnr_handle;

/* Derived per-joint constants of PioneerKinematicEnv.__init__
 * (pioneer_knm_env.py:56-61, :72, :217-220). */
typedef struct pnr_constants {
    float r_lo[PNR_DOF], r_hi[PNR_DOF]; /* joint_limits(), float32 */
    float v_max[PNR_DOF];               /* max_v_to_r * (r_hi - r_lo) */
    float a_max[PNR_DOF];               /* max_a_to_v * v_max == action_space bound */
    double dt;                          /* world.step_time = timestep * frame_skip */
    double eps;                         /* 1e-5 */
} pnr_constants;

/* PioneerKinematicConfig() / SimulationConfig() defaults. */
int pnr_config_default(pnr_config* cfg);

/* Constants derived from a config without creating a device handle. */
int pnr_get_constants(const pnr_config* cfg, pnr_constants* out);

/*
 * Replaces PioneerKinematicEnv.__init__ (pioneer_knm_env.py:39-74) +
 * BulletEnv.__init__/reset_simulator/load_scene (bullet_env.py:66-148) for
 * num_envs independent envs on HIP device `device_id`.  `env_id_offset` is the
 * global index of local env 0: the reset RNG is keyed by (seed, global env
 * id, episode#), so trajectories do not depend on how a batch is sharded
 * across GPUs.  The envs hold no valid state until the first full pnr_reset (mask == NULL) or
 * pnr_set_state: pnr_step / pnr_rollout / pnr_observe before that fail with PNR_ERR_INVALID
 * (the reference's constructor calls reset_world() itself, pioneer_knm_env.py:69; the Python
 * façade PioneerKinematicEnv does the same).
 */
int pnr_create(const pnr_config* cfg, int64_t num_envs, int64_t env_id_offset,
               int device_id, uint64_t seed, pnr_handle* out);

int pnr_destroy(pnr_handle h);

/* seed(): pioneer_knm_env.py:107-109.  Takes effect at the next reset. */
int pnr_seed(pnr_handle h, uint64_t seed);

/*
 * Replaces BulletEnv.reset (bullet_env.py:187-190) + reset_world
 * (pioneer_knm_env.py:76-105).
 *   mask        [num_envs] bytes, non-zero = reset this env; NULL = all
 *   joint_pos   [num_envs][6] env-major float32 or NULL — the reference's
 *               `joint_positions` override; NULL draws r ~ U(r_lo, r_hi)
 *   target_pos  [num_envs][3] env-major float32 or NULL — `target_position`
 *               override; NULL draws target ~ U(target_lo, target_hi)
 *   obs_out     obs batch in cfg.obs_layout, or NULL; rows of envs that are
 *               not reset are left untouched
 */
int pnr_reset(pnr_handle h, const uint8_t* mask, const float* joint_pos,
              const float* target_pos, float* obs_out, void* stream);

/*
 * Replaces BulletEnv.step (bullet_env.py:192-197) = act
 * (pioneer_knm_env.py:111-182) + observe (:184-211) + TimeLimit.step for every
 * env of the batch, in one kernel launch.
 *   actions    [num_envs x 6] float32 in cfg.action_layout
 *   obs        [num_envs x 137] float32 in cfg.obs_layout
 *   reward     [num_envs] float32
 *   done       [num_envs] bytes — the env's own `done` (distance < done_distance)
 *   truncated  [num_envs] bytes — TimeLimit.truncated (elapsed >= max && !done); may be NULL
 *   info       [num_envs][4] float32 (r_pot, r_step, r_done, dist) or NULL
 */
int pnr_step(pnr_handle h, const float* actions, float* obs, float* reward,
             uint8_t* done, uint8_t* truncated, float* info, void* stream);

/*
 * T consecutive steps in ONE launch with open-loop actions (state stays in
 * registers between steps).  Buffers are the pnr_step ones with a leading
 * [T] axis: actions [T][N x 6], obs [T][N x 137], reward/done/truncated [T][N].
 * Same results as T calls of pnr_step: bit for bit in kinematic mode; in dynamics mode
 * the simulated quantities agree to float32 rounding (two kernels, contraction allowed),
 * command state, counters, targets and per-env draws bit for bit.
 */
int pnr_rollout(pnr_handle h, int32_t T, const float* actions, float* obs,
                float* reward, uint8_t* done, uint8_t* truncated, void* stream);

/* observe() without stepping (pioneer_knm_env.py:184-211). */
int pnr_observe(pnr_handle h, float* obs_out, void* stream);

/*
 * World.step() (bullet_scene.py:273-275: frame_skip x stepSimulation) on its own: the simulator advances by step_time and
 * NOTHING else happens — no command integration, reward, TimeLimit, reset or observation.  What the reference's demo loop
 * drives (pioneer_knm_env.py:277-296: reset_state(position(), velocity); world.step()).
 *   dynamics-mode handle (joint_state must be NULL): frame_skip articulated-body sub-steps on the handle's simulated joints
 *     (q, qd of pnr_get_dyn_state) under gravity, contacts, joint limits, friction / damping and each joint's motor — the one
 *     pnr_set_joint_motor gave it, else the handle's own motor law tracking the env's command state r, v (teleport handles:
 *     no motor: the joints coast).  Parity unpinned, like all of dynamics mode.
 *   kinematic-mode handle: there is no simulated state; joint_state [num_envs][12] (q[6] | qd[6], float32, caller-owned
 *     device memory) is the joints as Bullet holds them after resetJointState(position, velocity), and with the reference's
 *     defaults (no gravity, no motor torque, no collision shapes) a step carries each on at its velocity: q += qd * step_time,
 *     stopped at its limit with the velocity zeroed.  The env's own state is not touched (the reference's self.r / self.v
 *     are not either).
 */
int pnr_world_step(pnr_handle h, float* joint_state, void* stream);

/*
 * Joint.control_position / Joint.control_velocity (bullet_scene.py:123-155 -> setJointMotorControl2) for joint `joint`
 * (0..5, URDF order) of every env of a dynamics-mode handle, honoured by pnr_world_step; pnr_step keeps driving every joint from
 * the env's own command state (the reference's act() teleports the joints each step, pioneer_knm_env.py:148).  Host-side and
 * synchronous: takes effect with the next pnr_world_step.  Parity unpinned.  Two laws:
 *
 * PD torque (PNR_CONTROL_POSITION: targetPosition, targetVelocity, positionGain, velocityGain, force, maxVelocity;
 * PNR_CONTROL_VELOCITY: targetVelocity, force).  An optional argument left out (NaN) takes the handle's configured value (pd_kp,
 * pd_kd, torque_limit, max_velocity; targetVelocity: 0).  The engine's one law (pnr_config.control_mode's folding, per joint):
 *   tau = clip(Kp (r* - q) + kd (clamp(v* + c (r* - q), +-maxVelocity) - qd), +-force);   force <= 0: no cap.
 *
 * Bullet's constraint motor (PNR_CONTROL_POSITION_CONSTRAINT: targetPosition required; PNR_CONTROL_VELOCITY_CONSTRAINT:
 * targetVelocity required).  Each sub-step of length h = timestep, the joint's torque is the one that brings its velocity to
 *   VELOCITY: rhs = v*        POSITION: rhs = clamp(Kp (r* - q) / h + qd + Kd (v* - qd), +-maxVelocity)  (maxVelocity > 0)
 * at the end of the sub-step, limited to |tau| <= force, solved jointly with the other constraint joints over the coupled chain
 * (gravity, contacts, damping, friction and the PD joints' torques all included).  Arguments left out (NaN) take Bullet's values
 * (PNR_BULLET_*), not the handle's.  force = 0 means NO motor: the joint is free (PD law: force <= 0 means no cap).
 * PNR_ERR_INVALID, with the motor left as it was, for a NaN or inf required target, an inf targetVelocity, a negative force or a
 * negative or non-finite gain.
 */
int pnr_set_joint_motor(pnr_handle h, int32_t joint, int32_t control_mode, double target_position, double target_velocity,
                        double position_gain, double velocity_gain, double max_force, double max_velocity);

/*
 * Raw state for checkpoint / tests, as planar 32-bit words [24][num_envs]:
 * words 0-5 a, 6-11 v, 12-17 r, 18-20 target, 21 potential (float32),
 * 22 step_index, 23 episode (uint32).  Device pointers.
 */
int pnr_get_state(pnr_handle h, uint32_t* words_out, void* stream);
int pnr_set_state(pnr_handle h, const uint32_t* words_in, void* stream);

/* Dynamics-mode extra state, planar float32 [36][num_envs]: q[6], qd[6],
 * link-mass scale[11], friction[6], damping[6], 1 pad.  PNR_ERR_UNSUPPORTED in
 * kinematic mode. */
int pnr_get_dyn_state(pnr_handle h, float* words_out, void* stream);
int pnr_set_dyn_state(pnr_handle h, const float* words_in, void* stream);

/*
 * Item.pose() / Item.velocity() of every link item (bullet_scene.py:53-67 -> getLinkState(computeLinkVelocity=1,
 * computeForwardKinematics=1)) for every env, in one launch: the world pose and velocity of each URDF link.
 *   out          [num_envs][PNR_NUM_LINKS][PNR_LINK_STATE_DIM] float32, row-major, 16-byte aligned; nothing past
 *                num_envs * 143 floats is written.  Record of link k:
 *                  [0:3]   world position of the link frame              (LinkState.link_world_position)
 *                  [3:7]   world orientation, quaternion (x, y, z, w), unit norm, w >= 0   (link_world_orientation)
 *                  [7:10]  world linear velocity of the link frame origin (world_link_linear_velocity)
 *                  [10:13] world angular velocity                         (world_link_angular_velocity)
 *                Link k is Bullet's link_index = the URDF joint order: robot:base, rotator1, hinge1, arm1, arm2,
 *                rotator2, hinge2, arm3, rotator3, effector, pointer.  Link 0 (robot:base) is static: identity at the
 *                origin, zero velocity.  Every link's inertial origin is its link frame origin and every fixed joint
 *                has rpy 0, so the link frame is Bullet's COM frame and its velocity the COM velocity.
 *   joint_state  [num_envs][12] float32 (q[6] | qd[6], the pnr_world_step layout), 16-byte aligned, read only: pure
 *                kinematics of the given joints, either mode.  NULL: the handle's own joints — dynamics mode the
 *                simulated q, qd (pnr_get_dyn_state words 0-11); kinematic mode the env's r and v (pnr_get_state
 *                words 12-17 and 6-11; PNR_ERR_INVALID before the first pnr_reset or pnr_set_state).
 * Any finite joint value is accepted (full-range sin/cos); non-finite input gives non-finite records, unchecked.
 * float32 arithmetic.  Parity unpinned (Bullet's own link states are not reproduced bit for bit).
 */
int pnr_get_link_states(pnr_handle h, const float* joint_state, float* out, void* stream);

/*
 * calculateJacobian for link `link` (0..10, Bullet's link_index as in pnr_get_link_states) of every env, one launch.
 *   local_point  HOST pointer to 3 doubles, a point in the link's frame (PyBullet's localPosition); NULL = the frame origin
 *   joint_state  as pnr_get_link_states ([num_envs][12] q | qd, 16-byte aligned, only q is read); NULL = the handle's own
 *                joints (PNR_ERR_INVALID before the first pnr_reset or pnr_set_state)
 *   out          [num_envs][6][6] float32 row-major, 16-byte aligned; nothing past num_envs * PNR_JACOBIAN_DIM floats is written.
 *                rows 0-2: world linear velocity of the point per unit velocity of joint j (column j, URDF revolute order);
 *                rows 3-5: world angular velocity of the link per unit velocity of joint j.
 *                Columns of joints that are not between the base and the link are exactly 0; link 0 gives all zeros.
 * So out . qd is the link's velocity as pnr_get_link_states reports it (at the point), and tau = J^T f maps a world force
 * at the point to joint torques.  Any finite joint value is accepted; non-finite input gives non-finite output, unchecked.
 * PNR_ERR_INVALID, nothing launched and no output touched, for: a null handle or out, link outside 0..10, a non-finite
 * local_point, misaligned pointers.  float32 arithmetic, asynchronous on `stream`, no allocation: capturable into a graph.
 */
int pnr_get_jacobian(pnr_handle h, const float* joint_state, int32_t link, const double* local_point, float* out, void* stream);

/*
 * Position-only inverse kinematics (calculateInverseKinematics without an orientation) for every env, one launch: joint
 * angles inside the URDF limits that put a point of a link on a world target.  Plain damped least squares; per env,
 * independently of every other env (an env's result does not depend on the batch around it, bit for bit):
 *
 *     q  = clamp(q_init, r_lo, r_hi)
 *     repeat up to max_iterations times:
 *         e = target - p(q);   stop (frozen from now on) if |e| <= tolerance        (float32 distance)
 *         J = the three linear rows of the Jacobian at q                          (3 x 6, as pnr_get_jacobian)
 *         y = (J J^T + lambda^2 I)^-1 e                                           (3 x 3, symmetric positive definite)
 *         dq = J^T y;   dq *= min(1, max_step / max_j |dq_j|)
 *         q = clamp(q + dq, r_lo, r_hi)
 *
 *   target_pos  [num_envs][3] float32 world positions, or NULL = each env's own target (pnr_get_state words 18-20;
 *               PNR_ERR_INVALID before the first pnr_reset or pnr_set_state)
 *   q_init      [num_envs][6] float32, or NULL = the rest pose q = 0; clamped into the joint limits before the first iteration
 *   q_out       [num_envs][6] float32 (8-byte aligned), always inside [r_lo, r_hi] of pnr_get_constants
 *   residual_out [num_envs] float32 or NULL: |target - point(q_out)| as the kernel's float32 forward kinematics sees it
 *   iterations_out [num_envs] int32 or NULL: iterations this env took (max_iterations if it never met the tolerance)
 *
 * Measured basin (float64 restatement of the chain, default parameters): from the rest pose every target of the box
 * (15, -8, 2) .. (22, 8, 6) converges in <= 7 iterations; from uniformly random starts inside the limits 17-23 % of the solves
 * end in a local minimum at a joint limit.  That is why NULL means the rest pose and not the env's current pose.  About 3 %
 * of the reference's target box (15, -10, 2) .. (25, 10, 6) cannot be reached at all (its far corners, |t| >= 25.4); from the
 * rest pose alone about 4 % of it is not reached (one target in a hundred stops in a local minimum of that start).
 *
 * PNR_ERR_INVALID, nothing launched and no output touched, for: a null handle, params or q_out, a wrong struct_size, link
 * outside 0..10, max_iterations outside 1..1024, a non-finite or non-positive damping or max_step, a negative or non-finite
 * tolerance, a non-finite local_point, misaligned pointers (q_out 8 bytes, the others 4).  Non-finite joint or target values
 * give non-finite outputs, unchecked; the loop is bounded by max_iterations.  float32 arithmetic, asynchronous on `stream`,
 * no allocation, no synchronisation: capturable into a graph.
 */
typedef struct pnr_ik_params {
    uint32_t struct_size;     /* sizeof(pnr_ik_params) */
    int32_t  link;            /* 0..10; default 10 (robot:pointer) */
    double   local_point[3];  /* a point in the link's frame; default 0 */
    int32_t  max_iterations;  /* 1..1024; default 32 */
    int32_t  reserved;
    double   damping;         /* lambda > 0, default 1.0 */
    double   max_step;        /* > 0, rad: cap on the largest joint change of one iteration, default 0.5 */
    double   tolerance;       /* >= 0: an env stops once its float32 distance is <= tolerance; default 1e-3 */
} pnr_ik_params;
int pnr_ik_params_default(pnr_ik_params* p);
int pnr_solve_ik(pnr_handle h, const pnr_ik_params* p, const float* target_pos, const float* q_init,
                 float* q_out, float* residual_out, int32_t* iterations_out, void* stream);

/*
 * Pose inverse kinematics (calculateInverseKinematics(..., targetOrientation=...)) for every env, one launch: joint angles inside
 * the URDF limits that put a point of a link on a world target AND turn the link to a target orientation (mode
 * PNR_IK_ORIENT_FULL), or point one axis of the link along the target's (PNR_IK_ORIENT_AXIS: the roll about the axis stays
 * free).  Damped least squares on the 6 x 6 system, the damping growing with the error; per env, independently of every other env
 * (an env's result does not depend on the batch around it, bit for bit):
 *
 *     q  = clamp(q_init, r_lo, r_hi)
 *     repeat up to max_iterations times:
 *         e_p = target_pos - p(q)                                                 (the point of the link, as pnr_solve_ik)
 *         (s, c) = sine vector and cosine of the rotation still to make, R(q) the link's world rotation:
 *             FULL: s = 1/2 sum_k r_k x t_k, c = (sum_k r_k . t_k - 1) / 2        (r_k, t_k: columns of R(q), R_target; s is the
 *                   vector of the antisymmetric part of R_target R(q)^T)
 *             AXIS: s = u x v, c = u . v                                          (u = R(q) a, v = R_target a, a = local_axis)
 *         angle = atan2(|s|, c) in [0, pi];   e_o = s angle / max(|s|, 1e-12)     (a world-frame rotation vector, rad)
 *         stop (frozen from now on) if |e_p| <= tolerance and angle <= angle_tolerance        (float32)
 *         e = [e_p ; w e_o];   J = [J_lin ; w J_ang]                              (w = orientation_weight, length per rad)
 *         lambda^2 = damping^2 + error_damping (|e_p|^2 + w^2 angle^2)
 *         y = (J J^T + lambda^2 I)^-1 e                                           (6 x 6, symmetric positive definite; L D L^T
 *                                                                                  with every pivot held at >= lambda^2)
 *         dq = J^T y;   dq *= min(1, max_step / max_j |dq_j|)
 *         q = clamp(q + dq, r_lo, r_hi)
 *
 * Where the rotation axis cannot be formed (half a turn in FULL mode, opposite vectors in AXIS mode: |s| = 0 with c < 0) the
 * max() makes the orientation step zero: outputs stay finite, `angle` stays pi, and the position part still moves the arm.
 * The damping is error-scaled because the rest pose is a wrist singularity (joints 4 and 6 are collinear at q5 = 0): far from
 * the target the step is cautious, near it the iteration is almost Gauss-Newton.
 *
 *   target_pos   [num_envs][3] float32 world positions, or NULL = each env's own target (PNR_ERR_INVALID before the first
 *                pnr_reset or pnr_set_state)
 *   target_quat  [num_envs][4] float32 (x, y, z, w), required; normalised by the kernel, the sign of w does not matter
 *   q_init       [num_envs][6] float32, or NULL = the rest pose q = 0; clamped into the joint limits before the first iteration
 *   q_out        [num_envs][6] float32 (8-byte aligned), always inside [r_lo, r_hi] of pnr_get_constants
 *   residual_out [num_envs] float32 or NULL: |target_pos - point(q_out)| as the kernel's float32 forward kinematics sees it
 *   angle_out    [num_envs] float32 or NULL: the angle left (rad), as the kernel sees it
 *   iterations_out [num_envs] int32 or NULL: iterations this env took (max_iterations if it never met both tolerances)
 *
 * Measured basin (float64 restatement of the law, default parameters, 4 096 poses per set): starts within +-0.2 rad per joint
 * of a solution whose |q5| >= 0.4 converge 100 % in <= 8 iterations (99 % in <= 4); AXIS-mode pointing along world +x anywhere
 * in the box (15, -8, 2) .. (22, 8, 6) converges 100 % from the rest pose in <= 6 iterations.  From the rest pose to the full
 * pose of random joints at 0.8-0.9 of the limits 88 % converge (the rest stop in local minima at joint limits or on the other
 * wrist branch; pnr_solve_ik_multi searches from several starts); with lambda = 1 and no error term (pnr_solve_ik's damping) only 74-76 % do,
 * and 98 % of the near starts.  orientation_weight 1, 3, 10, 30 give 94, 91, 88, 89 % from the rest pose and 100 % near.
 *
 * PNR_ERR_INVALID, nothing launched and no output touched, for: a null handle, params, q_out or target_quat, a wrong
 * struct_size, link outside 0..10, a mode outside {0, 1}, max_iterations outside 1..1024, a non-finite or non-positive damping,
 * max_step or orientation_weight, a negative or non-finite error_damping, tolerance or angle_tolerance, a non-finite local_point,
 * a non-finite or zero local_axis, misaligned pointers (q_out 8 bytes, the others 4), target_pos NULL before the first reset.
 * Non-finite targets give non-finite residuals, unchecked; the loop is bounded by max_iterations.  float32 arithmetic,
 * asynchronous on `stream`, no allocation, no synchronisation: capturable into a graph.
 */
enum pnr_ik_orient {
    PNR_IK_ORIENT_FULL = 0,   /* the link's full orientation */
    PNR_IK_ORIENT_AXIS = 1    /* only local_axis is aligned with the target's; the roll about it is free */
};
typedef struct pnr_ik_pose_params {
    uint32_t struct_size;       /* sizeof(pnr_ik_pose_params) */
    int32_t  link;              /* 0..10; default 10 (robot:pointer) */
    double   local_point[3];    /* a point in the link's frame; default 0 */
    int32_t  max_iterations;    /* 1..1024; default 32 */
    int32_t  mode;              /* PNR_IK_ORIENT_FULL (default) or PNR_IK_ORIENT_AXIS */
    double   local_axis[3];     /* AXIS mode: the axis in the link's frame, any length > 0 (normalised by the host); default (1, 0, 0) */
    double   damping;           /* > 0, default 0.03 */
    double   error_damping;     /* >= 0, default 0.01 */
    double   orientation_weight; /* w > 0, length per rad, default 10 */
    double   max_step;          /* > 0, rad: cap on the largest joint change of one iteration, default 0.5 */
    double   tolerance;         /* >= 0, length; default 1e-3 */
    double   angle_tolerance;   /* >= 0, rad; default 1e-3 */
} pnr_ik_pose_params;
int pnr_ik_pose_params_default(pnr_ik_pose_params* p);
int pnr_solve_ik_pose(pnr_handle h, const pnr_ik_pose_params* p, const float* target_pos, const float* target_quat, const float* q_init,
                      float* q_out, float* residual_out, float* angle_out, int32_t* iterations_out, void* stream);

/*
 * Multi-start inverse kinematics for every env, one launch: S descents per env from S starts, and of the solutions found the one
 * nearest to a posture.  Each start runs the law of pnr_solve_ik (task PNR_IK_TASK_POSITION) or of pnr_solve_ik_pose (task
 * PNR_IK_TASK_POSE: its FULL mode; PNR_IK_TASK_AXIS: its AXIS mode) exactly as stated above, with the one damping
 *
 *     lambda^2 = damping^2 + error_damping (|e_p|^2 + w^2 angle^2)                 (the position task has no orientation rows:
 *                                                                                  angle = 0, and its default error_damping is 0)
 *
 * A start's iterates do not depend on S, on the env's other starts (policy BEST) or on any other env, bit for bit: start k of
 * an S-start call ends where a one-start call from the same joints ends.
 *
 *   starts       num_starts = S in {1, 2, 4, 8, 16, 32, 64}.  `starts` is [S][6] float32, one table for all envs, or, with
 *                starts_per_env != 0, [num_envs][S][6]; NULL only with S = 1 (start 0 is then q_init, else the rest pose).
 *                q_init [num_envs][6] or NULL: where given it replaces start 0 of every env.  Every start is clamped into the
 *                joint limits before the first iteration.
 *   converged    a start is converged when the pose it ends at is within the tolerances (float32; the position task: the distance)
 *   selection    per env, over its S starts when the env stops: the smallest (not converged, cost, start index),
 *                lexicographically.  cost of a converged start: sum_j (q_j - q_ref_j)^2, q_ref [num_envs][6] or NULL = the env's
 *                clamped start 0; of a start that is not converged: |e_p| + w angle (the position task: |e_p|).  A cost that is
 *                not finite counts as +inf, so the order is total: a NaN target selects start 0, with non-finite residuals.
 *   policy       PNR_IK_MULTI_BEST: every start runs until it converges or max_iterations is reached; the winner is the converged
 *                start nearest to q_ref.  PNR_IK_MULTI_FIRST: at the convergence check in which any start of an env converges
 *                all of that env's starts freeze; the winner is the nearest of the starts that converged in that check (no start
 *                converges: as BEST).  FIRST is there for the time of a wave, which under BEST nearly always holds a lane that
 *                runs max_iterations.
 *   outputs      of the winner: q_out [num_envs][6] (8-byte aligned, required), and optionally residual_out, angle_out (0 in the
 *                position task), iterations_out, start_out (int32: the winner's start index), each [num_envs];
 *                converged_out [num_envs] int32 or NULL: how many of the env's starts are converged when it stops (0: none).
 *                Per start, each optional: all_q [num_envs][S][6] (8-byte aligned), all_residual, all_angle, all_iterations
 *                [num_envs][S] — every branch found.  Under FIRST a start frozen by another's convergence reports the
 *                iterations it made.  Nothing past these extents is written.
 *
 * PNR_ERR_INVALID, nothing launched and no output touched (the message names the field), for: everything pnr_solve_ik (position
 * task) or pnr_solve_ik_pose (pose and axis tasks) refuses, a negative or non-finite error_damping in any task, an unknown task
 * or policy, a num_starts outside the seven values, NULL starts with num_starts > 1, NULL target_quat in a pose or axis task, a
 * NULL or wrongly sized buffers struct, misaligned pointers (q_out and all_q 8 bytes, the others 4).  float32 arithmetic,
 * asynchronous on `stream`, no allocation, no synchronisation: capturable into a graph.
 */
enum pnr_ik_task {
    PNR_IK_TASK_POSITION = 0,   /* pnr_solve_ik's 3 x 3 law */
    PNR_IK_TASK_POSE = 1,       /* pnr_solve_ik_pose, PNR_IK_ORIENT_FULL */
    PNR_IK_TASK_AXIS = 2        /* pnr_solve_ik_pose, PNR_IK_ORIENT_AXIS */
};
enum pnr_ik_multi_policy {
    PNR_IK_MULTI_BEST = 0,      /* the nearest of all converged starts */
    PNR_IK_MULTI_FIRST = 1      /* the nearest of the starts that converge first */
};
typedef struct pnr_ik_multi_params {
    uint32_t struct_size;       /* sizeof(pnr_ik_multi_params) */
    int32_t  task;              /* pnr_ik_task */
    int32_t  policy;            /* pnr_ik_multi_policy; default PNR_IK_MULTI_BEST */
    int32_t  num_starts;        /* S: 1, 2, 4, 8, 16, 32 or 64; default 8 */
    int32_t  starts_per_env;    /* 0 (default): `starts` is [S][6]; else [num_envs][S][6] */
    int32_t  link;              /* 0..10; default 10 (robot:pointer) */
    double   local_point[3];    /* a point in the link's frame; default 0 */
    int32_t  max_iterations;    /* 1..1024; default 32 */
    int32_t  reserved;
    double   local_axis[3];     /* axis task: as pnr_ik_pose_params.local_axis; default (1, 0, 0) */
    double   damping;           /* > 0; default 1.0 (position), 0.03 (pose, axis) */
    double   error_damping;     /* >= 0; default 0 (position), 0.01 (pose, axis) */
    double   orientation_weight; /* w > 0, pose and axis tasks; default 10 */
    double   max_step;          /* > 0, rad; default 0.5 */
    double   tolerance;         /* >= 0, length; default 1e-3 */
    double   angle_tolerance;   /* >= 0, rad, pose and axis tasks; default 1e-3 */
} pnr_ik_multi_params;
typedef struct pnr_ik_multi_buffers {
    uint32_t struct_size;       /* sizeof(pnr_ik_multi_buffers) */
    uint32_t reserved;
    const float* target_pos;    /* [num_envs][3], or NULL = each env's own target (as pnr_solve_ik) */
    const float* target_quat;   /* [num_envs][4] (x, y, z, w); pose and axis tasks, not read in the position task */
    const float* starts;        /* [S][6] or [num_envs][S][6]; NULL only with num_starts 1 */
    const float* q_init;        /* [num_envs][6] or NULL */
    const float* q_ref;         /* [num_envs][6] or NULL */
    float*   q_out;             /* [num_envs][6], 8-byte aligned */
    float*   residual_out;      /* [num_envs] or NULL */
    float*   angle_out;         /* [num_envs] or NULL */
    int32_t* iterations_out;    /* [num_envs] or NULL */
    int32_t* start_out;         /* [num_envs] or NULL */
    int32_t* converged_out;     /* [num_envs] or NULL */
    float*   all_q;             /* [num_envs][S][6], 8-byte aligned, or NULL */
    float*   all_residual;      /* [num_envs][S] or NULL */
    float*   all_angle;         /* [num_envs][S] or NULL */
    int32_t* all_iterations;    /* [num_envs][S] or NULL */
} pnr_ik_multi_buffers;
int pnr_ik_multi_params_default(pnr_ik_multi_params* p, int32_t task);
int pnr_solve_ik_multi(pnr_handle h, const pnr_ik_multi_params* p, const pnr_ik_multi_buffers* b, void* stream);

/*
 * calculateInverseDynamics for every env, one launch: the joint torques of
 *     tau = M(q) qdd + C(q, qd) qd + G(q)
 * on the rigid-body model the dynamics mode steps (six merged moving bodies; oracle/pnr_dyn_oracle.h describes it), by
 * recursive Newton-Euler.  Gravity is the handle's pnr_config.gravity along -z.
 *   joint_state  [num_envs][12] float32 (q[6] | qd[6]), 16-byte aligned, read only, as pnr_get_link_states; NULL = the handle's
 *                own joints (dynamics mode the simulated q, qd; kinematic mode the env's r and v)
 *   joint_accel  [num_envs][6] float32 qdd, 16-byte aligned, read only; NULL = qdd 0: the bias forces C qd + G (with qd = 0 as
 *                well: the gravity torques G(q))
 *   flags        PNR_INVDYN_NO_GRAVITY leaves G(q) out.  PNR_INVDYN_JOINT_LOSSES adds the engine's joint damping and smoothed
 *                Coulomb friction at qd, damping_i qd_i + friction_i qd_i / sqrt(qd_i^2 + 0.05^2): the torque is then exactly
 *                what a sub-step of the engine needs to realise qdd away from contacts and joint limits.  Without it the call is
 *                PyBullet's: no damping, friction, contacts, motors or limits.  Any other bit: PNR_ERR_INVALID.
 *   out          [num_envs][6] float32 env-major, 16-byte aligned; nothing past num_envs * 6 floats is written
 * Link masses: on a dynamics-mode handle the per-env link scales of its dyn state (pnr_get_dyn_state words 12-22) and, for the
 * losses, its per-env friction and damping (words 23-34), whatever the joint source; on a kinematic-mode handle every scale is 1
 * and the losses use pnr_config.joint_friction / joint_damping.  PNR_ERR_INVALID before the first pnr_reset (or pnr_set_state /
 * pnr_set_dyn_state): on a dynamics-mode handle always (the scales do not exist yet), on a kinematic-mode one with a NULL
 * joint_state.  PNR_ERR_INVALID, nothing launched and no output touched, also for a null handle or out, misaligned pointers or
 * unknown flag bits.  Non-finite input gives non-finite output, unchecked.  float32 arithmetic, asynchronous on `stream`, no
 * allocation: capturable into a graph.  Parity unpinned.
 */
#define PNR_INVDYN_NO_GRAVITY   1   /* leave G(q) out */
#define PNR_INVDYN_JOINT_LOSSES 2   /* add the engine's joint damping and smoothed Coulomb friction at qd */
int pnr_inverse_dynamics(pnr_handle h, const float* joint_state, const float* joint_accel, int32_t flags, float* out, void* stream);

/*
 * calculateMassMatrix for every env, one launch: the joint-space inertia M(q) of the same model (composite rigid bodies).
 *   joint_state  as pnr_inverse_dynamics; only q is read
 *   out          [num_envs][6][6] float32 row-major, 16-byte aligned: the full symmetric matrix, both triangles written from one
 *                computed value (out[i][j] == out[j][i] bit for bit); nothing past num_envs * 36 floats is written
 * Joint sources, link masses, refusals and conventions as pnr_inverse_dynamics.
 */
int pnr_mass_matrix(pnr_handle h, const float* joint_state, float* out, void* stream);

/*
 * pnr_world_step on a dynamics-mode handle with a joint torque per env (PyBullet's TORQUE_CONTROL).
 *   joint_torques  [num_envs][6] float32 env-major, caller-owned device memory, 16-byte aligned, read only.  The torque is added
 *                  to each joint's torque in every sub-step of THIS call, after the motor law's own cap and before damping and
 *                  friction; it lasts this call only and must be given again for the next step, as in Bullet.
 * The joints' motors stay as pnr_set_joint_motor left them and act as well: a caller who wants pure torque control first gives
 * the joints zero gains (PNR_CONTROL_VELOCITY with velocity_gain 0, the PD law), as one disables Bullet's default motor with
 * force 0.  PNR_ERR_UNSUPPORTED: a kinematic-mode handle; a motor table that holds a constraint motor (PNR_CONTROL_*_CONSTRAINT:
 * torque input together with the boxed solve is not built).  PNR_ERR_INVALID: a null handle, NULL or misaligned joint_torques,
 * before the first pnr_reset.  Nothing is launched and the state is untouched on every refusal.  Asynchronous on `stream`, no
 * allocation: capturable into a graph.  Parity unpinned.
 */
int pnr_world_step_torques(pnr_handle h, const float* joint_torques, void* stream);

/*
 * pnr_world_step on a dynamics-mode handle with the caller's wrenches on links of the arm: PyBullet's applyExternalForce /
 * applyExternalTorque for every env, in the world step's own launch.  One call is one World.step (frame_skip sub-steps of length
 * timestep) exactly as pnr_world_step_torques, with n_specs <= PNR_MAX_LINK_WRENCHES wrench records per env.
 *
 * Record j.  Call-uniform: specs[j] = {link, frame} (host memory, read during the call).  link is 0..10, the index of
 * pnr_get_link_states; frame is PNR_FRAME_LINK or PNR_FRAME_WORLD (pybullet's LINK_FRAME = 1 and WORLD_FRAME = 2 as recalled, not
 * verified against a PyBullet install).  Per env: nine floats of wrenches, force[3] | position[3] | torque[3].
 *
 * The URDF link maps to its dynamic body b (the six moving bodies, fixed joints merged) with the link origin's fixed offset d in
 * body coordinates (0 for every link but robot:pointer, which sits at (3.6, 0, 1.9) in the last body).  The URDF's fixed joints
 * carry no rotation, so link axes are body axes.  Link 0 (robot:base) is welded to the world: a record on it is accepted and
 * does nothing.
 *   PNR_FRAME_LINK   force, torque and position are in the link's frame (= Bullet's link COM frame: the inertial origins are
 *                    identity) and turn with the link.  In body coordinates, constant over the call:
 *                      f_b = force,   n_b = (d + position) x force + torque
 *   PNR_FRAME_WORLD  force and torque stay fixed in the world for the whole call; position is a world point, and the wrench acts
 *                    on the material point of the link that lies there at the pose q0 of the call's start:
 *                      p_b = R_b(q0)^T (position - o_b(q0)), fixed afterwards;
 *                    in sub-step k, with the body's rotation at its start:  f_b = R_b(q_k)^T force,
 *                      n_b = p_b x f_b + R_b(q_k)^T torque
 * fext[b] += (n_b, f_b), summed over the records and added to the contact wrenches where the handle has contacts; it is
 * subtracted from the body's bias force in the articulated-body recursion, as the contacts are.  Motor law, caps, damping,
 * friction, joint limits and the integrator are untouched.
 *   hold_substeps  the records act in the first hold_substeps sub-steps of the call; <= 0 or >= frame_skip: all of them (the
 *                  force lasts one World.step).  1 is Bullet's literal behaviour under the reference's World.step (external
 *                  forces are cleared after one stepSimulation).  Nothing persists after the call.
 *   wrenches       [num_envs][n_specs][9] float32, caller-owned device memory, 16-byte aligned, read only
 *   joint_torques  [num_envs][6] float32, 16-byte aligned, read only, or NULL for none: exactly pnr_world_step_torques' torques,
 *                  in the same launch (a computed-torque controller under a disturbance is one call)
 * PNR_ERR_UNSUPPORTED: a kinematic-mode handle; a motor table that holds a constraint motor (as pnr_world_step_torques).
 * PNR_ERR_INVALID: a null handle, NULL specs or wrenches, misaligned wrenches or joint_torques, n_specs outside
 * 1..PNR_MAX_LINK_WRENCHES, a link outside 0..10, an unknown frame, before the first pnr_reset.  Every refusal is decided before
 * any launch and leaves the state untouched.  Device data is not inspected: a NaN or inf in wrenches gives that env non-finite
 * joints and no error.  Asynchronous on `stream`, never synchronises, no allocation: capturable into a graph.  Parity unpinned:
 * the reference never applies a force; checked against the float64 oracle's forward dynamics with external body forces.
 */
#define PNR_MAX_LINK_WRENCHES 4
#define PNR_FRAME_LINK  1
#define PNR_FRAME_WORLD 2
typedef struct pnr_link_wrench_spec { int32_t link; int32_t frame; } pnr_link_wrench_spec;
int pnr_world_step_wrenches(pnr_handle h, const pnr_link_wrench_spec* specs, int n_specs, const float* wrenches,
                            const float* joint_torques, int hold_substeps, void* stream);

/*
 * pnr_world_step on a dynamics-mode handle with motor targets of each env's own: PyBullet's setJointMotorControlArray followed by
 * stepSimulation, once per env.  One call is one World.step (frame_skip sub-steps on the handle's simulated q, qd) exactly as
 * pnr_world_step, but for every joint j with bit j of joint_mask set, env e's motor of joint j takes, for THIS call only,
 *     targetPosition = targets[e][j],   targetVelocity = targets[e][6 + j]
 * in place of what the motor table holds for that joint (pnr_set_joint_motor's target_position / target_velocity).
 *   joint_mask     bits 0..5, at least one set
 *   targets        [num_envs][12] float32, position[6] | velocity[6] (the q | qd layout of every joint_state argument of this
 *                  header), caller-owned device memory, 16-byte aligned, read only.  The entries of joints outside joint_mask take
 *                  no part in the result and may hold anything, NaN included.
 *   joint_torques  [num_envs][6] float32, 16-byte aligned, read only, or NULL for none: exactly pnr_world_step_torques' torques,
 *                  in the same launch
 * Everything else about joint j's motor stays as pnr_set_joint_motor left it and is the same for all envs: the law (PD position,
 * PD velocity or a constraint motor), the gains, the force cap, maxVelocity.  A masked joint nobody commanded keeps the handle's
 * own law (pnr_config.control_mode, pd_kp, pd_kd, torque_limit, max_velocity) with the env's targets standing in for its command
 * state r[j], v[j]; on a teleport handle such a joint has no motor and its targets do nothing, and neither do those of a constraint
 * motor set with force == 0 (no motor).  Joints outside joint_mask behave exactly as in pnr_world_step.  The position entry of a
 * joint on a velocity law has no effect on the result; under the PD velocity law it is multiplied by a zero gain, so it must be
 * FINITE (a NaN or inf there gives that env non-finite joints).  Device data is not inspected and no error is raised for it.
 * Nothing persists after the call: the command state, the motor table and every dyn word but q, qd are left bit for bit.
 *
 * Contract: for every env e the call gives what pnr_world_step (with joint_torques: pnr_world_step_torques) gives env e on a
 * handle in the same state whose motor table holds env e's entries as the targets of the masked joints — to float32 rounding, the
 * two being different kernels.  An env's result does not depend on the batch around it, bit for bit.
 * PNR_ERR_UNSUPPORTED: a kinematic-mode handle; joint_torques non-NULL with a constraint motor anywhere in the table (as
 * pnr_world_step_torques: torque input together with the boxed solve is not built).  PNR_ERR_INVALID: a null handle, NULL or
 * misaligned targets, misaligned joint_torques, joint_mask == 0 or with a bit above 5, before the first pnr_reset.  Every refusal
 * is decided before any launch and leaves the state untouched.  Asynchronous on `stream`, never synchronises, no allocation:
 * capturable into a graph.  Parity unpinned: checked per env against the float64 oracle's world step and the constraint motor's
 * float64 reference under that env's table.
 */
int pnr_world_step_targets(pnr_handle h, uint32_t joint_mask, const float* targets, const float* joint_torques, void* stream);

/*
 * ONE MOVING SPHERE per env, in dynamics mode: createMultiBody(baseMass > 0) with a sphere collision shape (bullet_scene.py:230-246,
 * Scene.create_body_sphere :193-204), and the base-item branch of Item.pose / velocity / reset_pose (getBasePositionAndOrientation,
 * getBaseVelocity, resetBasePositionAndOrientation, bullet_scene.py:53-73).  The world step integrates the sphere together with
 * the arm; it collides with the arm's contact samples and with everything static.  It is a POINT MASS WITH A RADIUS: position and
 * linear velocity, no orientation, no spin — ROLLING IS NOT MODELLED.  Boxes and planes stay static.
 *
 * State: the handle owns a planar float32 buffer [PNR_BODY_STATE_WORDS][num_envs]: words 0-2 the world position of the centre,
 * 3-5 the linear velocity, 6 the mass, 7 the radius.  Mass and radius are per env (they can be randomised).  AN ENV WHOSE MASS
 * WORD IS <= 0 HAS NO SPHERE: it exerts and feels no force, and its eight words are never written.
 *
 * The law.  Per sub-step of length h = timestep, every force is evaluated at the state the sub-step starts from; kp, kd are the
 * params' contact_kp, contact_kd; x, v, m, radius the env's words.
 *   Sphere against the static world (ground_z, the obstacle box, the n_scene bodies), always surface to surface: with sdf the signed
 *   distance of the centre to the body's surface (positive outside; the signed-distance forms of the arm's contacts) and n the
 *   outward normal there, depth = radius - sdf, fn = kp depth - kd (v . n); where depth > 0 and fn > 0 the force is
 *       fn n - friction fn v_t / sqrt(|v_t|^2 + slip_eps^2),    v_t = v - (v . n) n      (regularised sliding friction).
 *   Sphere against the arm: the arm's samples are the pointer's sample sphere always and all 23 with link_contacts.  For a sample
 *   with centre p_s, velocity v_s and radius r_s: d = x - p_s, len = |d|, depth = radius + r_s - len, n = d / len ((0, 0, 1) at
 *   len == 0), fn = kp depth - kd ((v - v_s) . n); where depth > 0 and fn > 0, +fn n acts on the sphere and -fn n on the sample, where
 *   it enters the sample's body exactly as a static contact force does.  There is no friction between arm and sphere.
 *   Integration (semi-implicit Euler, as the joints'): v += h (F / m - linear_damping v - gravity z^), x += h v.
 * Stability of the explicit penalty spring needs contact_kd timestep < mass and contact_kp timestep^2 < mass: with the defaults
 * (50, 2000, 1/240) that is mass > 0.21.  Mass and radius are device data and cannot be validated on the host.
 *
 * pnr_body_params: contact_kp, contact_kd NaN = the handle's (pnr_config.contact_kp / contact_kd); friction 0.5; slip_eps 0.05;
 * linear_damping 0 (pnr_body_params_default).
 * pnr_set_body_params enables the sphere.  Its first call on a handle allocates the buffer and zero-fills it — every env inert
 * until a state is set — and WAITS for that fill (Conventions: the second synchronising exception); later calls only replace the
 * params.  params == NULL disables the sphere and keeps the buffer and its contents.  PNR_ERR_UNSUPPORTED: a kinematic-mode handle.
 * PNR_ERR_INVALID: a null handle, a wrong struct_size, contact_kp <= 0, contact_kd / friction / linear_damping < 0, slip_eps <= 0,
 * anything non-finite.
 * pnr_set_body_state writes words [8][num_envs] (device memory, 16-byte aligned, read only) into the buffer with one small kernel;
 * with mask ([num_envs] bytes, device memory) only the envs with a non-zero byte — the device-side "reset the sphere of the envs
 * that just finished".  pnr_get_body_state copies the buffer to out [8][num_envs] (16-byte aligned).  Both are asynchronous on
 * `stream`, never synchronise and allocate nothing; PNR_ERR_INVALID before the first pnr_set_body_params, for a null or misaligned
 * pointer.  They work while the sphere is disabled.
 *
 * With a sphere enabled pnr_world_step, pnr_world_step_torques and pnr_world_step_targets move it (same signatures, same checks, one
 * launch: the kernels' forms with the sphere, always with contact code).  Not built, and refused with PNR_ERR_UNSUPPORTED in a message
 * that names the sphere: any of them with a constraint motor in the table, pnr_world_step_wrenches, pnr_get_joint_states.
 * pnr_step, pnr_rollout and pnr_reset neither move nor see the sphere.  Parity unpinned; checked against a float64 restatement of
 * this law on the float64 oracle's forward dynamics.
 */
typedef struct pnr_body_params {
    uint32_t struct_size;
    float contact_kp, contact_kd;
    float friction;
    float slip_eps;
    float linear_damping;
} pnr_body_params;
int pnr_body_params_default(pnr_body_params* p);
int pnr_set_body_params(pnr_handle h, const pnr_body_params* params);
int pnr_set_body_state(pnr_handle h, const float* words, const uint8_t* mask, void* stream);
int pnr_get_body_state(pnr_handle h, float* out, void* stream);

/*
 * THE GRIP: each env's moving sphere held at a point of link robot:pointer, PyBullet's createConstraint(arm, pointerLink, body, -1,
 * JOINT_POINT2POINT, ...) with changeConstraint(maxForce) — how suction and magnet grippers are modelled — removeConstraint and
 * getConstraintState.  Dynamics mode, on a handle with a sphere buffer (pnr_set_body_params first).
 *
 * State: the handle owns a planar float32 buffer [PNR_BODY_GRIP_WORDS][num_envs]: word 0 the env's max_force (<= 0: released, the
 * state after allocation), words 1-3 the world-frame force on the sphere in the last sub-step of the last world step.
 *
 * The law: a soft point-to-point constraint with a force cap between a point of the pointer link and the sphere's centre,
 * evaluated in every sub-step at the state the sub-step starts from, as every other force of the world step is, in every env whose
 * max_force word is > 0 and whose mass word is > 0.  With R_5, p_5 the world pose of moving body 5 (the last one, which carries
 * the pointer), (omega, v_lin) its spatial velocity in its own coordinates, kTip = (3.6, 0, 1.9) the pointer's origin in that body,
 * radius_e the env's radius word and x, v the sphere's centre and velocity:
 *     c_a = kTip + anchor + (radius_e + pointer_radius) direction      (body 5's frame; anchor and direction are the params')
 *     p_a = p_5 + R_5 c_a,   v_a = R_5 (v_lin + omega x c_a)           (as a contact sample's position and velocity)
 *     e   = x - p_a,   e'  = v - v_a
 *     F_r = - grip_kp e - grip_kd e'
 *     F   = F_r min(1, max_force / |F_r|)        (F = F_r where |F_r| <= max_force, in particular at F_r = 0)
 * +F acts on the sphere, next to the static world's force, before the sphere's integration; -F acts on body 5 at c_a and enters it
 * exactly as a contact reaction does.  The force is continuous in the state everywhere (no normalised direction, no threshold).
 * WHILE AN ENV IS GRIPPED ITS SPHERE TAKES NO ARM-SPHERE CONTACT FROM ANY SAMPLE: the held sphere may overlap the pointer.  Its
 * contacts with the static world stay, so it can be lifted off the ground and set down on a box.  A released env (max_force <= 0)
 * follows the sphere's law above exactly, arm contacts included.
 * Stability of the explicit spring needs grip_kp timestep^2 < m and grip_kd timestep < m, with m the smaller of the sphere's mass
 * and the arm's effective mass at the pointer: with the defaults (2000, 50, 1/240) that is m > 0.21, as for the contacts.
 *
 * pnr_body_grip_params (pnr_body_grip_params_default): anchor (0, 0, 0); direction the unit vector along the tip offset
 * (3.6, 0, 1.9) in the pointer's frame, with which the held sphere sits tangent to the pointer's own sample sphere for any per-env
 * radius, so that a release does not start from a deep penetration; direction (0, 0, 0) makes the anchor a plain point of the link;
 * any other direction is normalised.  grip_kp, grip_kd NaN = the sphere's resolved contact_kp, contact_kd at the time of the call.
 * pnr_set_body_grip_params enables the grip.  Its first call on a handle allocates the buffer and zero-fills it — every env
 * released — and WAITS for that fill, as the first pnr_set_body_params does; later calls only replace the params.  params == NULL
 * disables the grip and keeps the buffer: the world step then launches the kernels of a handle that never knew a grip.
 * pnr_set_body_grip writes max_force [num_envs] (device memory, read only) into word 0 and zeros into words 1-3, for every env or,
 * with mask ([num_envs] bytes, device memory), the envs with a non-zero byte: the device-side "grip the envs that just came within
 * reach" or "drop the envs that just finished".  pnr_get_body_grip copies the buffer to out [4][num_envs] (16-byte aligned): words
 * 1-3 are PyBullet's getConstraintState.  The world step writes words 1-3 of gripped envs with mass > 0 and of no other.  Both
 * calls are asynchronous on `stream`, never synchronise and allocate nothing, and work while the grip is disabled.
 * PNR_ERR_UNSUPPORTED: a kinematic-mode handle.  PNR_ERR_INVALID: a null handle, a call before the first pnr_set_body_params, a
 * wrong struct_size, anything non-finite, grip_kp <= 0, grip_kd < 0, a direction that is neither zero nor normalisable, a null or
 * misaligned pointer, pnr_set_body_grip / pnr_get_body_grip before the first pnr_set_body_grip_params.  Every refusal is decided
 * before any launch and changes nothing.  max_force is device data and cannot be validated on the host (NaN counts as released).
 * What the sphere refuses stays refused, in the sphere's messages: constraint motors, pnr_world_step_wrenches, pnr_get_joint_states.
 * THE SCENE QUERIES DO NOT KNOW THE GRIP: pnr_get_contacts keeps reporting (and pricing) the overlap of a held sphere with the arm's
 * samples that the step ignores; pnr_render and pnr_ray_test see the sphere where it is, as before.  pnr_step, pnr_rollout and
 * pnr_reset neither move nor see the sphere, gripped or not.  Parity unpinned; checked against a float64 restatement of this law.
 */
typedef struct pnr_body_grip_params {
    uint32_t struct_size;
    float anchor[3], direction[3];
    float grip_kp, grip_kd;
} pnr_body_grip_params;
int pnr_body_grip_params_default(pnr_body_grip_params* p);
int pnr_set_body_grip_params(pnr_handle h, const pnr_body_grip_params* params);
int pnr_set_body_grip(pnr_handle h, const float* max_force, const uint8_t* mask, void* stream);
int pnr_get_body_grip(pnr_handle h, float* out, void* stream);

/*
 * Which of the batched scene queries SEE the moving sphere: pnr_render / pnr_render_bodies, pnr_ray_test, pnr_get_contacts.
 *   queries  PNR_BODY_IN_RENDER | PNR_BODY_IN_RAYS | PNR_BODY_IN_CONTACTS; 0, the state after pnr_create, is every query as it was
 *            before this call existed (the sphere is invisible to all three).
 *   rgba     4 host floats, the colour pnr_render draws the sphere in (rgb used, alpha ignored: opaque), or NULL = keep the current
 *            colour; initially the URDF's obstacle_mat, (0.3, 0.3, 0.3, 1).
 * A host-side switch stored in the handle: no launch, no allocation, no synchronisation; it holds for every later call on the
 * handle.  A query whose bit is set reads the handle's body-state buffer when it runs (so it sees what pnr_world_step and
 * pnr_set_body_state last wrote, in stream order): env k has a sphere where its mass word is > 0 (the step's own rule), centre words
 * 0-2, velocity 3-5, radius 7.  Whether pnr_set_body_params(NULL) has disabled the sphere for the step does not matter, and the
 * caller's joint_state combines freely with the handle's sphere.  What a set bit means is stated with each query below; in short:
 *   render    one more opaque sphere per env, segmentation label PNR_SEG_MOVING_BODY (21), shaded and depth-tested like a body
 *   rays      one more solid among the bodies (PNR_RAY_HIT_BODIES), label 21, after the caller's bodies on a tie
 *   contacts  one more body, index PNR_MAX_SCENE (8), with the step's arm-sphere law on the RELATIVE velocity
 * PNR_ERR_UNSUPPORTED: a kinematic-mode handle.  PNR_ERR_INVALID: a null handle, a call before the first pnr_set_body_params (there
 * is no buffer), unknown bits, a non-finite colour.  A refused call changes nothing.
 */
enum pnr_body_query { PNR_BODY_IN_RENDER = 1, PNR_BODY_IN_RAYS = 2, PNR_BODY_IN_CONTACTS = 4 };
int pnr_set_body_queries(pnr_handle h, uint32_t queries, const float* rgba);

/*
 * getJointState for every env of a dynamics-mode handle, one launch: per revolute joint its position, velocity, ACCELERATION and
 * MOTOR TORQUE, and optionally the joint's REACTION WRENCH.  The call evaluates exactly what the FIRST SUB-STEP of
 * pnr_world_step, pnr_world_step_torques or pnr_world_step_wrenches would evaluate if called with the same arguments, and takes
 * nothing: no word of the state is written.  It reads the joints, the handle's command state r, v, the motor table as
 * pnr_set_joint_motor left it, the per-env link scales, friction and damping, and the handle's contacts.
 *   joint_state    as pnr_get_link_states ([num_envs][12] q | qd, 16-byte aligned, read only); NULL = the handle's simulated q, qd
 *   joint_torques  [num_envs][6] float32, 16-byte aligned, read only, or NULL: pnr_world_step_torques' torques
 *   specs, n_specs, wrenches
 *                  up to PNR_MAX_LINK_WRENCHES wrench records per env: specs, layout ([num_envs][n_specs][9], 16-byte aligned) and
 *                  frames are pnr_world_step_wrenches'.  A PNR_FRAME_WORLD record's point is taken on the link at the current
 *                  pose, which is that call's q0.  n_specs == 0 with NULL specs and NULL wrenches: no records.
 *   joints_out     [num_envs][6][4] float32, 16-byte aligned: q, qd, qdd, tau_motor per joint; nothing past num_envs * 24 floats
 *                  is written.
 *                  qdd is the acceleration the sub-step would integrate: the articulated-body algorithm's output, after the boxed
 *                  solve where the table holds constraint motors, BEFORE the integrator and its joint-limit clamp.  The clamp is
 *                  a select of the integrator (q held at the limit, qd zeroed) and not a force: it shows in neither output.
 *                  tau_motor is what the joint's own motor applies: the PD table law's torque after its cap; under
 *                  pd_inertia_scaled the scaled and capped torque clip(D_i ades_i, +-cap) the recursion applies; for a constraint
 *                  motor the boxed solve's torque.  It contains neither the caller's joint_torques nor damping nor friction.
 *   reaction_out   [num_envs][6][6] float32, 16-byte aligned, or NULL (not computed); nothing past num_envs * 36 floats is
 *                  written.  Per revolute joint b: (Fx, Fy, Fz, Mx, My, Mz), the wrench the PARENT body exerts ON body b through
 *                  the joint, taken AT body b's origin (which lies on the joint axis) and expressed IN body b's coordinates:
 *                  the child link's frame, since the URDF's fixed joints carry no rotation and the inertial origins are identity.
 *                  Bodies are the six merged moving bodies.  It carries everything distal to the joint: the inertial forces of
 *                  bodies b..5 at qdd and gravity, minus the contact wrenches and the caller's wrenches on them.  Its moment along
 *                  the joint axis is the joint's total torque, tau_motor + joint_torque - damping - friction; the other five
 *                  components are the bearing load.  An arm at rest under gravity shows (0, 0, +weight) at joint 0.  Sign and
 *                  frame against Bullet's jointReactionForces are unpinned, as everything in dynamics mode.
 * The refusals are the world-step calls', so that "same arguments, same answer" holds.  PNR_ERR_UNSUPPORTED: a kinematic-mode
 * handle (nothing is simulated there); joint_torques or wrench records with a motor table that holds a constraint motor.
 * PNR_ERR_INVALID: a null handle or joints_out; a misaligned pointer; n_specs outside 0..PNR_MAX_LINK_WRENCHES, n_specs > 0 with
 * NULL specs or wrenches, n_specs == 0 with either of them; a link outside 0..10; an unknown frame; before the first pnr_reset.
 * Every refusal is decided before any launch and touches no output.  Device data is not inspected.  float32 arithmetic,
 * asynchronous on `stream`, never synchronises, no allocation: capturable into a graph.  Parity unpinned; checked against the
 * float64 oracle's forward dynamics and a world-frame Newton-Euler sweep over the URDF's links.
 */
int pnr_get_joint_states(pnr_handle h, const float* joint_state, const float* joint_torques, const pnr_link_wrench_spec* specs,
                         int32_t n_specs, const float* wrenches, float* joints_out, float* reaction_out, void* stream);

/*
 * getContactPoints / getClosestPoints for every env, one launch: each of the arm's 23 contact sample spheres against up to
 * PNR_MAX_SCENE static bodies given with the call (as pnr_render's: a kinematic-mode handle can ask too).
 *   Samples: the sample spheres the dynamics mode collides with link_contacts (oracle/pnr_dyn_oracle.h describes them: 8 on
 *   arm1, 7 on arm2, 2 on rotator2 + hinge2, 3 on arm3, 3 on the effector's needle), in that order; sample 22 is the pointer's
 *   sphere, of pnr_config.pointer_radius.  Always all 23, each with its SURFACE against each body's surface.  The signed
 *   distance forms are the step's for scene bodies: plane, sphere, oriented box (inside a box: out through the nearest face).
 *   The step's one quirk is NOT part of the query: with link_contacts = 0 the step lets the pointer meet ground_z with its
 *   centre; here the pointer, too, touches with its surface.
 *   joint_state     as pnr_get_link_states ([num_envs][12] q | qd, 16-byte aligned, read only); NULL = the handle's own joints
 *                   (dynamics mode the simulated q, qd; kinematic mode the env's r and v)
 *   p               the bodies (shape, position, orientation, size as in pnr_config.scene; body index = position in this
 *                   list) and the penalty law's gains contact_kp, contact_kd
 *   body_positions  [num_envs][n_bodies][3] float32 or NULL: a world position per env that replaces bodies[b].position for
 *                   that env (orientation and size stay shared): the per-env obstacle.  Ignored when n_bodies == 0.
 *   points          [num_envs][PNR_CONTACT_SAMPLES][PNR_CONTACT_DIM] float32 or NULL.  The record of sample s, against the
 *                   nearest body (smallest signed distance; the lower index on a tie):
 *                     [0]   signed distance, surface to surface (< 0: penetrating); +inf when n_bodies == 0
 *                     [1:4] unit world normal on the body towards the sample (contactNormalOnB); 0 when n_bodies == 0
 *                     [4:7] world position on the sample's surface, centre - radius n (positionOnA); the position on the
 *                           body (positionOnB) is [4:7] - [0] n
 *                     [7]   that body's index as a float; -1 when n_bodies == 0
 *                     [8]   that body's normal force on the sample: max(0, kp depth - kd (v . n)) if depth = -distance > 0,
 *                           else 0; v is the sample centre's world velocity from qd
 *   summary         [num_envs][4] float32 or NULL: the smallest distance over the samples, that sample's index (the lowest
 *                   on a tie; 0 when n_bodies == 0), that sample's body, the number of samples with distance < 0
 *   joint_torques   [num_envs][6] float32 or NULL: tau_c = sum_s J_s(q)^T F_s, F_s the sum over ALL bodies of the force above
 *                   on sample s (what the step accumulates): joint j's entry is a_j . ((pos_s - o_j) x F_s) over the samples
 *                   outboard of it.  pnr_world_step_torques with these on a contact-free handle is a step with contacts.
 *   The moving sphere (a handle with PNR_BODY_IN_CONTACTS set, pnr_set_body_queries): in every env whose mass word is > 0 the
 *   sphere is one more body, index PNR_MAX_SCENE (8) in points[..][7] and summary[2].  With x, v, radius the env's words and p_s,
 *   v_s, r_s the sample's centre, velocity and radius: distance = |p_s - x| - radius - r_s (surface to surface), the normal on
 *   the sphere towards the sample n = (p_s - x) / |p_s - x|, (0, 0, -1) at zero distance (the mirror of the step's (0, 0, 1)), and
 *   the force max(0, kp depth - kd ((v_s - v) . n)) where depth = -distance > 0: the step's arm-sphere law, with this call's
 *   contact_kp, contact_kd and the RELATIVE velocity.  F_s, and so joint_torques, include it.  The sphere competes for "nearest
 *   body" with the caller's bodies and, having the highest index, loses a tie.  With n_bodies == 0 an env with a sphere reports
 *   the sphere; an env without one reports what it reports without the bit.
 * At least one output must be non-NULL; nothing is written past num_envs rows of any output; outputs 16-byte aligned,
 * body_positions 4-byte.  An env's results do not depend on the batch around it, bit for bit.
 * PNR_ERR_INVALID, nothing launched and no output touched, for: a null handle or params, a wrong struct_size, n_bodies outside
 * 0..PNR_MAX_SCENE, a bad shape or non-finite / degenerate body data (as pnr_render), negative or non-finite gains, misaligned
 * pointers, all outputs NULL, a NULL joint_state before the first pnr_reset (or pnr_set_state).  Non-finite joint values or
 * body_positions give non-finite output, unchecked.  float32 arithmetic, asynchronous on `stream`, no allocation, no
 * synchronisation: capturable into a graph.  Parity unpinned: Bullet's narrow phase and manifolds are not reproduced (one point
 * per sample, against analytic shapes).
 */
#define PNR_CONTACT_SAMPLES 23      /* the sample spheres, in table order; sample 22 is the pointer */
#define PNR_CONTACT_DIM 9
typedef struct pnr_contact_params {
    uint32_t struct_size;                    /* sizeof(pnr_contact_params) */
    int32_t  n_bodies;                       /* 0 .. PNR_MAX_SCENE */
    double   contact_kp, contact_kd;         /* the penalty law's gains, finite and >= 0; default pnr_config's 2000, 50 */
    pnr_scene_body bodies[PNR_MAX_SCENE];    /* as pnr_config.scene / pnr_render_params.bodies */
} pnr_contact_params;
int pnr_contact_params_default(pnr_contact_params* p);
int pnr_get_contacts(pnr_handle h, const float* joint_state, const pnr_contact_params* p,
                     const float* body_positions, float* points, float* summary,
                     float* joint_torques, void* stream);

/*
 * Path clearance for every env, one launch: the arm swept along a piecewise-linear joint path, each configuration's clearance
 * to the bodies of the call (pnr_get_contacts' distances, without its velocities, normals and forces) and the path's summary.
 * The edge check of a sampling planner, the shield of a joint-target action, the score of a set of IK candidates.
 * THIS IS A SAMPLED CHECK: only the C configurations below are looked at.  Something thinner than the samples' travel between
 * two neighbouring configurations can be missed; choose substeps for the joint step the scene needs.
 *   The path.  waypoints is [num_envs][K][6] float32 (waypoints_per_env != 0) or [K][6], shared by all envs (== 0), K =
 *   n_waypoints, 8-byte aligned.  With from_current != 0 the env's own joints are waypoint 0 in front of the K given ones
 *   (dynamics mode the simulated q, kinematic mode the env's r, as pnr_get_contacts reads them with a NULL joint_state).  W, the
 *   number of waypoints so obtained, must be >= 1; K = 0 (waypoints NULL) with from_current is the env where it stands.
 *   The configurations.  C = 1 + (W - 1) M, M = substeps.  Configuration 0 is waypoint 0; configuration 1 + i M + (j - 1),
 *   j = 1..M, lies on segment i from waypoint a to waypoint b: a + (j / M) (b - a) in float32 for j < M and EXACTLY b for j = M,
 *   so a waypoint's clearance is pnr_get_contacts' distance at that configuration.  Its path coordinate is t = i + j / M (0 for
 *   configuration 0).  M = 1 looks at the waypoints alone: a candidate set.
 *   The clearance of a configuration: the smallest signed surface-to-surface distance over the samples in sample_mask (bit s =
 *   sample s of pnr_get_contacts; the pointer, sample 22, at pnr_config.pointer_radius) and over all bodies, in
 *   pnr_get_contacts' forms; body_positions [num_envs][n_bodies][3] as there.  On a handle with PNR_BODY_IN_CONTACTS set
 *   (pnr_set_body_queries) the env's moving sphere is body PNR_MAX_SCENE (8), standing still where it is now; it loses a tie.
 *   A (sample, body) distance that is not finite counts as -inf: the order is total, and a NaN waypoint or body position makes
 *   the path not free.
 *   summary  [num_envs][PNR_PATH_SUMMARY_DIM] float32 or NULL, 16-byte aligned:
 *              [0] the smallest clearance over the path; [1] its path coordinate t (the lowest configuration on a tie);
 *              [2], [3] the sample and the body that attain it (within a configuration the lowest sample, then the lowest
 *              body, as in pnr_get_contacts); [4] t of the first configuration with clearance < margin, -1 if there is none;
 *              [5] the number of such configurations; [6] 1 if there is none, else 0; [7] 0.
 *            With n_bodies == 0 and no sphere: +inf, 0, 0, -1, -1, 0, 1, 0.
 *   clearance  [num_envs][C] float32 or NULL: every configuration's clearance, the profile.
 * At least one output must be non-NULL; nothing is written past num_envs rows of either.
 * lanes_per_env: how many lanes of a 64-lane wave share an env's configurations: 1, 2, 4, .. 64, or 0 = auto: the smallest
 * power of two >= C, at most 32 (at C = 81 and 65 536 envs 32 lanes measured 537 us against 64 lanes' 725 us: three trips of
 * 32 leave 15 lane-trips idle, two of 64 leave 47).  The outputs are bit-identical for every value, and an env's do not depend
 * on the batch around it.
 * PNR_ERR_INVALID, nothing launched and no output touched, for: everything pnr_get_contacts refuses about the handle, the
 * params' struct_size, n_bodies, the bodies and the pointers' alignment; n_waypoints outside 0..PNR_MAX_PATH_WAYPOINTS; substeps
 * outside 1..PNR_MAX_PATH_SUBSTEPS; a lanes_per_env that is none of the above; from_current or waypoints_per_env other than 0
 * or 1; n_waypoints 0 without from_current; NULL waypoints with n_waypoints > 0; a sample_mask with no bit among the 23 samples
 * or with a bit above them; a non-finite margin; every output NULL; from_current before the first pnr_reset (or
 * pnr_set_state).  Device data is not inspected.  float32 arithmetic, asynchronous on `stream`, no allocation, no
 * synchronisation: capturable into a graph.  Parity unpinned, as pnr_get_contacts.
 */
#define PNR_MAX_PATH_WAYPOINTS 256
#define PNR_MAX_PATH_SUBSTEPS 64
#define PNR_PATH_SUMMARY_DIM 8
typedef struct pnr_path_params {
    uint32_t struct_size;                    /* sizeof(pnr_path_params) */
    int32_t  n_waypoints;                    /* K: the given waypoints, 0 .. PNR_MAX_PATH_WAYPOINTS; default 1 */
    int32_t  substeps;                       /* M: configurations per segment, 1 .. PNR_MAX_PATH_SUBSTEPS; default 8 */
    int32_t  from_current;                   /* != 0: the env's own joints are waypoint 0 */
    int32_t  waypoints_per_env;              /* != 0: waypoints is [num_envs][K][6], else [K][6] */
    int32_t  lanes_per_env;                  /* 0 (auto), 1, 2, 4, 8, 16, 32, 64 */
    uint32_t sample_mask;                    /* bit s = sample s; default all 23 (0x7fffff) */
    int32_t  n_bodies;                       /* 0 .. PNR_MAX_SCENE */
    double   margin;                         /* a configuration with clearance < margin violates; finite; default 0 */
    pnr_scene_body bodies[PNR_MAX_SCENE];    /* as pnr_contact_params.bodies */
} pnr_path_params;
int pnr_path_params_default(pnr_path_params* p);
int pnr_path_clearance(pnr_handle h, const pnr_path_params* p, const float* waypoints, const float* body_positions,
                       float* summary, float* clearance, void* stream);

/*
 * Cartesian path inverse kinematics for every env, one call: the pointer (any link point) follows a piecewise-linear path of
 * poses in the WORLD, and the answer is the joint path that does it — PyBullet users' loop of calculateInverseKinematics(...,
 * currentPositions = previous) over interpolated targets.  Its q_path is what pnr_path_clearance (waypoints, C <= 256) and
 * pnr_world_step_targets (row by row) take.
 *   inputs     waypoint_pos is [num_envs][K][3] float32 (waypoints_per_env != 0) or [K][3], shared by all envs (== 0), K =
 *              n_waypoints in 1 .. PNR_MAX_PATH_WAYPOINTS.  Pose and axis tasks: waypoint_quat [num_envs][K][4] or [K][4], x, y, z,
 *              w.  M = substeps in 1 .. PNR_MAX_PATH_SUBSTEPS; C = 1 + (K - 1) M configurations.  task: pnr_ik_task, as in
 *              pnr_solve_ik_multi.  There is no "env's own target" form.
 *   targets    Configuration 0 is waypoint 0.  Configuration 1 + i M + (j - 1), j = 1 .. M, lies on segment i from waypoint a to
 *              waypoint b, u = (float)j / (float)M: position a + u (b - a) in float32 (each operation rounded once); orientation
 *              the normalised (1 - u) q_a + u h q_b, h = -1 if q_a . q_b < 0 else +1 (the dot product summed x, y, z, w; the
 *              shortest-arc nlerp: its squared norm is >= 1/2 for unit inputs, and the kernel normalises every target quaternion
 *              as pnr_solve_ik_multi does).  At j = M the target is EXACTLY waypoint b, by a select.
 *   starts     num_starts = S in {1, 2, 4, 8, 16, 32, 64}; starts, starts_per_env and q_init (replacing start 0) exactly as in
 *              pnr_solve_ik_multi, clamped into the limits.  S = 1 with q_init the env's own joints: "follow the line from where
 *              the arm stands".
 *   tracking   per start, independent of S, of the env's other starts and of every other env, bit for bit.  Configuration c
 *              runs the task's unchanged iteration (pnr_solve_ik_multi's, with lambda^2 = damping^2 + error_damping (|e_p|^2 +
 *              w^2 angle^2), max_step and the limit clamp) from the joints configuration c - 1 ended at; configuration 0 from
 *              the start.  The cap is max_iterations for configuration 0 and track_iterations for every later one.  A
 *              configuration is REACHED when the pose it ends at is within tolerance (and angle_tolerance in the pose and axis
 *              tasks).  A start STOPS at its first configuration that is not reached, c_fail, and makes no further iteration:
 *              its rows for c > c_fail are copies of row c_fail (joints, residual, angle) with iterations 0.  A start is TRACKED
 *              when every configuration is reached; then c_fail = -1.
 *   per start  travel = sum_j |q_0j - q_ref_j| (only with q_ref, [num_envs][6]) + sum_{c >= 1} sum_j |q_cj - q_(c-1)j|, float32,
 *              accumulated one term at a time with c ascending, then j ascending, over the configurations up to c_fail;
 *              max_jump = max over those c >= 1 of max_j |q_cj - q_(c-1)j| (0 for C = 1): a branch flip shows here.
 *   selection  per env the smallest (not tracked, cost, start index), lexicographically: a tracked start's cost is its travel,
 *              an untracked start's (float)(C - c_fail) — the start that got farthest wins.  A cost that is not finite counts as
 *              +inf, so the order is total.  A NaN waypoint makes its env untracked (c_fail: the first configuration whose target
 *              holds it) and leaves every other env's bits alone.
 *   outputs    summary [num_envs][PNR_IK_PATH_SUMMARY_DIM] float32, 16-byte aligned, required, of the winner: [0] tracked (1 / 0);
 *              [1] c_fail (-1: none); [2] the largest residual over configurations 0 .. c_fail (all when tracked; a residual
 *              that is not a number is the largest); [3] the largest angle over the same (0 in the position task); [4] travel;
 *              [5] max_jump; [6] the winner's start index; [7] the number of the env's tracked starts.
 *              q_path [num_envs][C][6] (8-byte aligned) or NULL: the winner's joints.  residual_path, angle_path [num_envs][C]
 *              float32, iterations_path [num_envs][C] int32, each or NULL: the winner's profile.
 *              all_summary [num_envs][S][4] float32 (16-byte aligned) or NULL, per start: tracked, c_fail, travel, max_jump.
 *              Nothing past these extents is written.  Every start's path is not an output.
 *   the winner's rows under S > 1 are written by tracking the winner's start a second time with the same code: THE WINNER'S ROWS
 *              OF AN S-START CALL EQUAL, BIT FOR BIT, THE ROWS OF A ONE-START CALL WHOSE q_init IS THAT START.  winner_rows
 *              chooses how: PNR_IK_PATH_ROWS_SECOND_PASS runs the configurations again inside the launch with only the winners'
 *              lanes live; PNR_IK_PATH_ROWS_SECOND_LAUNCH is a second launch of the same kernel at one lane per env, which reads
 *              the start index from `summary`; PNR_IK_PATH_ROWS_AUTO (default) is the second launch.  The same bits either way.
 * PNR_ERR_INVALID, nothing launched and no output touched (the message names the field), for: everything pnr_solve_ik_multi
 * refuses for the task (a NULL or wrongly sized params or buffers struct, task, num_starts, NULL starts with num_starts > 1,
 * link, the scalars, local_axis, misaligned pointers: summary and all_summary 16 bytes, q_path 8, the others 4); n_waypoints,
 * substeps, track_iterations or winner_rows out of range; NULL waypoint_pos or summary; NULL waypoint_quat in a pose or axis
 * task.  float32 arithmetic, asynchronous on `stream`, no allocation, no synchronisation: capturable into a graph.
 */
#define PNR_IK_PATH_SUMMARY_DIM 8
enum pnr_ik_path_rows {
    PNR_IK_PATH_ROWS_AUTO = 0,
    PNR_IK_PATH_ROWS_SECOND_PASS = 1,
    PNR_IK_PATH_ROWS_SECOND_LAUNCH = 2
};
typedef struct pnr_ik_path_params {
    uint32_t struct_size;       /* sizeof(pnr_ik_path_params) */
    int32_t  task;              /* pnr_ik_task */
    int32_t  num_starts;        /* S: 1, 2, 4, 8, 16, 32 or 64; default 1 */
    int32_t  starts_per_env;    /* 0 (default): `starts` is [S][6]; else [num_envs][S][6] */
    int32_t  n_waypoints;       /* K: 1 .. PNR_MAX_PATH_WAYPOINTS; default 1 */
    int32_t  waypoints_per_env; /* != 0: the waypoints are [num_envs][K][..], else [K][..] (default) */
    int32_t  substeps;          /* M: 1 .. PNR_MAX_PATH_SUBSTEPS; default 8 */
    int32_t  link;              /* 0..10; default 10 (robot:pointer) */
    int32_t  max_iterations;    /* configuration 0's cap, 1..1024; default 32 */
    int32_t  track_iterations;  /* every later configuration's cap, 1..1024; default 8 */
    int32_t  winner_rows;       /* pnr_ik_path_rows; default PNR_IK_PATH_ROWS_AUTO */
    int32_t  reserved;
    double   local_point[3];    /* a point in the link's frame; default 0 */
    double   local_axis[3];     /* axis task: as pnr_ik_pose_params.local_axis; default (1, 0, 0) */
    double   damping;           /* > 0; default 1.0 (position), 0.03 (pose, axis) */
    double   error_damping;     /* >= 0; default 0 (position), 0.01 (pose, axis) */
    double   orientation_weight; /* w > 0, pose and axis tasks; default 10 */
    double   max_step;          /* > 0, rad; default 0.5 */
    double   tolerance;         /* >= 0, length; default 1e-3 */
    double   angle_tolerance;   /* >= 0, rad, pose and axis tasks; default 1e-3 */
} pnr_ik_path_params;
typedef struct pnr_ik_path_buffers {
    uint32_t struct_size;       /* sizeof(pnr_ik_path_buffers) */
    uint32_t reserved;
    const float* waypoint_pos;  /* [K][3] or [num_envs][K][3] */
    const float* waypoint_quat; /* [K][4] or [num_envs][K][4] (x, y, z, w); pose and axis tasks, not read in the position task */
    const float* starts;        /* [S][6] or [num_envs][S][6]; NULL only with num_starts 1 */
    const float* q_init;        /* [num_envs][6] or NULL */
    const float* q_ref;         /* [num_envs][6] or NULL */
    float*   summary;           /* [num_envs][8], 16-byte aligned */
    float*   q_path;            /* [num_envs][C][6], 8-byte aligned, or NULL */
    float*   residual_path;     /* [num_envs][C] or NULL */
    float*   angle_path;        /* [num_envs][C] or NULL */
    int32_t* iterations_path;   /* [num_envs][C] or NULL */
    float*   all_summary;       /* [num_envs][S][4], 16-byte aligned, or NULL */
} pnr_ik_path_buffers;
int pnr_ik_path_params_default(pnr_ik_path_params* p, int32_t task);
int pnr_solve_ik_path(pnr_handle h, const pnr_ik_path_params* p, const pnr_ik_path_buffers* b, void* stream);

/*
 * Time parameterisation of every env's joint path, one call: WHEN the arm should be at which row of a q_path, rest to rest,
 * as fast as the joints' velocity, acceleration and (PNR_RETIME_TORQUE) torque limits allow.  The reachability-analysis form of
 * time-optimal path parameterisation: a backward pass of controllable sets, then a greedy forward pass.  pnr_sample_trajectory
 * turns the result into the [n][T][12] rows of q | qd that pnr_world_step_targets takes, one row per world step.
 *   path       points p_k in R^6, k = 0 .. C - 1, C = n_points in 3 .. PNR_MAX_TRAJ_POINTS: q_path [num_envs][C][6]
 *              (path_per_env != 0) or [C][6], shared; float32, 8-byte aligned — what pnr_solve_ik_path writes and
 *              pnr_path_clearance reads.  The path coordinate s has grid spacing 1 and q(s) is the linear interpolation between
 *              grid points.  C = 2 is refused: with x_0 = x_1 = 0 it cannot move under this discretisation.
 *   differences, one float32 operation each: d_0 = p_1 - p_0, d_(C-1) = p_(C-1) - p_(C-2), else d_k = (p_(k+1) - p_(k-1)) / 2;
 *              e_0 = e_(C-1) = 0, else e_k = (p_(k+1) - 2 p_k) + p_(k-1).
 *   unknowns   x_k = sdot^2 at grid point k; u_k = sddot, constant on interval k (k to k + 1): x_(k+1) = x_k + 2 u_k; rest to
 *              rest, x_0 = x_(C-1) = 0.
 *   rows       at grid point k = 0 .. C - 2, each |A u + B x + c| <= LIM.  Acceleration, joint j: A = d_kj, B = e_kj, c = 0,
 *              LIM = a_max[j].  Torque, joint j (PNR_RETIME_TORQUE): A = ID(p_k, 0, d_k) and B = ID(p_k, d_k, e_k) without
 *              gravity, c = ID(p_k, 0, 0) with the handle's gravity, LIM = tau_max[j]; ID(q, qd, qdd) is pnr_inverse_dynamics
 *              without joint losses (a dynamics-mode handle: the env's link scales; a kinematic one: the nominal model).
 *              Velocity: x <= X_k = min over the joints with d_kj != 0 of (v_max[j] / |d_kj|)^2 (the quotient, then its
 *              square); DECIDED HERE: a grid point where no joint moves (d_k = 0) has X_k = 0 — the path has no speed there.
 *   backward   K_(C-1) = 0; for k = C - 2 .. 0: K_k = max { x in [0, X_k] : a u exists with every row at k and
 *              0 <= x + 2u <= K_(k+1) }, evaluated without a division by A: each row's sign is turned so that A >= 0 (A, B, c
 *              negated where A < 0) and gives a lower line A u >= L - B x, L = -LIM - c, and an upper line A u <= H - B x,
 *              H = LIM - c; the next state adds the line A = 2, B = 1, L = 0, H = K_(k+1).  Every ordered pair (lower line i,
 *              upper line j), i != j (a line with itself says 0 <= 2 A LIM), gives slope x <= rhs with slope = A_i B_j - A_j B_i,
 *              rhs = A_i H_j - A_j L_i (each two products and a difference): slope > 0 bounds x above by rhs / slope, slope < 0
 *              below, slope == 0 with rhs < 0 makes the set empty.  K_k = the smallest upper bound and X_k; the set is empty
 *              too when the largest lower bound, or 0, exceeds K_k, and at k = 0 when a lower bound is > 0 (x_0 = 0 must lie in
 *              it).  7 lines without torque rows, 13 with them.
 *   forward    x_0 = 0; u = min over the rows with A > 0 of ((LIM - c) - B x_k) / A (none: +inf); x_(k+1) = min(max(x_k + 2u, 0),
 *              K_(k+1)); the reported u_k = (x_(k+1) - x_k) / 2.
 *   times      t_0 = 0, t_(k+1) = t_k + 2 / (sqrt(x_k) + sqrt(x_(k+1))), float32, k ascending.
 *   infeasible an env is infeasible, with k_fail and a pnr_retime_reason, when: a K_k is empty (PNR_RETIME_EMPTY; e.g. |G|
 *              exceeds tau_max where the arm must be held or lifted: the limits cannot even hold it there) or a coefficient or
 *              K_k at k is not finite (PNR_RETIME_NONFINITE) — the backward pass reports the first such k it meets, which is
 *              the LARGEST; or an interval has sqrt(x_k) + sqrt(x_(k+1)) = 0 (PNR_RETIME_STUCK, the smallest such k): three or
 *              more equal rows in a run, such as the tail pnr_solve_ik_path repeats after c_fail, or an interior stop that
 *              lasts an interval.  A NaN point makes its own env infeasible and leaves every other env's bits alone; an env's
 *              result never depends on the batch around it, nor on path_per_env, bit for bit.
 *   outputs    summary [num_envs][PNR_RETIME_SUMMARY_DIM] float32, 16-byte aligned, required: [0] feasible (1 / 0); [1] the
 *              duration t_(C-1), +inf when infeasible; [2] k_fail (-1 when feasible); [3] the reason; [4] sqrt of the largest
 *              x_k; [5] the largest row utilisation |(A u_k + B x_k) + c| / LIM over the rows and k = 0 .. C - 2; [6], [7] 0.
 *              times, sdot2 [num_envs][C] float32, each or NULL: t_k and x_k.  Rows of an infeasible env: after a backward
 *              failure (EMPTY, NONFINITE) no forward pass counts — sdot2 is 0 everywhere, times is 0 at k = 0 and +inf after,
 *              [4] = [5] = 0; when STUCK the whole forward profile is in sdot2 (and in [4], [5]) and times holds t_k for
 *              k <= k_fail and +inf after.
 *   workspace  only with PNR_RETIME_TORQUE: pnr_retime_workspace_bytes bytes (n_points x 18 x num_envs floats; 0 without the
 *              flag), 4-byte aligned, the caller's; it holds the torque rows A[6] | B[6] | c[6] planar, [C][18][num_envs].
 *   what it is first-order collocation: the rows hold at the grid points for (x_k, u_k).  The result is feasible by
 *              construction and time-optimal only as the grid is refined.  ON A COARSE GRID THE GREEDY PASS CAN BRING x TO 0 AT
 *              AN INTERIOR POINT — a stop; a float64 prototype did so on about a third of 17- and 33-point sinusoid paths and on
 *              none of 256 points.  Not built: boundary speeds other than rest, jerk limits, corner blending, per-env limit
 *              vectors, C > PNR_MAX_TRAJ_POINTS.
 * pnr_sample_trajectory: targets [num_envs][n_samples][12] float32, 16-byte aligned, n_samples in 1 .. PNR_MAX_TRAJ_SAMPLES.
 * Sample i is at tau = t0 + (float)(i + 1) dt (float32: the product, then the sum); k is the interval with t_k <= tau < t_(k+1),
 * delta = tau - t_k, sigma = sqrt(x_k) delta + (u_k delta^2) / 2 clamped to [0, 1], q = p_k + sigma (p_(k+1) - p_k),
 * qd = (p_(k+1) - p_k)(sqrt(x_k) + u_k delta), u_k = (x_(k+1) - x_k) / 2.  At and past the duration (summary[1]) the row is
 * p_(C-1) | 0: it holds.  For an infeasible env (summary[0] == 0) every row is p_0 | 0.  t0 >= 0, dt > 0.  A row is exactly what
 * pnr_world_step_targets takes for all six joints; windows t0 = 0, T dt, 2 T dt, .. tile a trajectory.
 * Both calls: PNR_ERR_INVALID, nothing launched and no output touched (the message names the field), for a NULL or wrongly sized
 * struct, n_points, path_per_env, flags, a limit in use that is not finite and > 0 (also as float32), n_samples, t0, dt, a NULL
 * required pointer (q_path, summary; workspace with the flag; every pointer of pnr_sample_trajectory) or a misaligned one
 * (summary, targets 16 bytes; q_path 8; the others 4); with PNR_RETIME_TORQUE on a dynamics-mode handle before its first reset.
 * float32 arithmetic, asynchronous on `stream`, no allocation, no synchronisation: capturable into a graph.  Both kinds of handle.
 */
#define PNR_MAX_TRAJ_POINTS 256
#define PNR_MAX_TRAJ_SAMPLES 65536
#define PNR_RETIME_SUMMARY_DIM 8
#define PNR_RETIME_ROW_DIM 18
enum pnr_retime_flags {
    PNR_RETIME_TORQUE = 1
};
enum pnr_retime_reason {
    PNR_RETIME_FEASIBLE = 0,
    PNR_RETIME_EMPTY = 1,
    PNR_RETIME_STUCK = 2,
    PNR_RETIME_NONFINITE = 3
};
typedef struct pnr_retime_params {
    uint32_t struct_size;       /* sizeof(pnr_retime_params) */
    int32_t  n_points;          /* C: 3 .. PNR_MAX_TRAJ_POINTS; default 3 */
    int32_t  path_per_env;      /* 1: q_path is [num_envs][C][6]; 0 (default): [C][6], shared */
    int32_t  flags;             /* pnr_retime_flags; default 0 */
    double   v_max[6];          /* rad/s, > 0; default 2 */
    double   a_max[6];          /* rad/s^2, > 0; default 10 */
    double   tau_max[6];        /* joint torque, > 0 with PNR_RETIME_TORQUE (not read without); default 0: to be set */
} pnr_retime_params;
typedef struct pnr_retime_buffers {
    uint32_t struct_size;       /* sizeof(pnr_retime_buffers) */
    uint32_t reserved;
    const float* q_path;        /* [C][6] or [num_envs][C][6], 8-byte aligned */
    void*    workspace;         /* pnr_retime_workspace_bytes bytes with PNR_RETIME_TORQUE, else not read (NULL is fine) */
    float*   summary;           /* [num_envs][8], 16-byte aligned */
    float*   times;             /* [num_envs][C] or NULL */
    float*   sdot2;             /* [num_envs][C] or NULL */
} pnr_retime_buffers;
typedef struct pnr_traj_sample_params {
    uint32_t struct_size;       /* sizeof(pnr_traj_sample_params) */
    int32_t  n_points;          /* C of the timed path */
    int32_t  path_per_env;      /* as pnr_retime_params */
    int32_t  n_samples;         /* T: 1 .. PNR_MAX_TRAJ_SAMPLES; default 1 */
    double   t0;                /* >= 0; default 0 */
    double   dt;                /* > 0; default 10 / 240 (pnr_config_default's timestep x frame_skip: one world step) */
} pnr_traj_sample_params;
int pnr_retime_params_default(pnr_retime_params* p);
int pnr_retime_workspace_bytes(pnr_handle h, const pnr_retime_params* p, uint64_t* bytes);
int pnr_retime_path(pnr_handle h, const pnr_retime_params* p, const pnr_retime_buffers* b, void* stream);
int pnr_traj_sample_params_default(pnr_traj_sample_params* p);
int pnr_sample_trajectory(pnr_handle h, const pnr_traj_sample_params* p, const float* q_path, const float* times, const float* sdot2,
                          const float* summary, float* targets, void* stream);

/*
 * render('rgb_array') for every env in one launch (bullet_env.py:156-185 -> getCameraImage): one camera shared by all envs,
 * each env's scene drawn by ray casting against analytic shapes.
 *   Scene of env k: the URDF's 14 <visual> shapes (boxes, cylinders, the pointer's sphere; their <material> colours) posed by
 *   the env's joints; the target, a sphere of pnr_config.target_radius at the env's target (pnr_get_state words 18-20); the
 *   caller's n_bodies static bodies, shared by all envs (planes are infinite).
 *   joint_state: as pnr_get_link_states ([num_envs][12] q | qd, 16-byte aligned, read only; NULL = the handle's own joints:
 *   dynamics mode the simulated q, kinematic mode the env's r).
 *   Camera: view is world -> eye, row-major 4x4 (render.view_matrix): the eye looks along -z with +y up; its 3x3 part must be
 *   orthonormal (to 1e-5) and its last row is ignored.  Pixel (x, y), row 0 at the top, is the ray through
 *   ndc (2(x + 0.5)/W - 1, 1 - 2(y + 0.5)/H) under the vertical-fov_y perspective of aspect W/H (render.project).
 *   Hit rule: per primitive, the entering and the leaving intersection are both candidates; a candidate counts if its eye depth
 *   lies in (near_clip, far_clip); the nearest opaque candidate wins.  The target is the one translucent surface: if it is
 *   nearer than the opaque hit, colour = a c_target + (1 - a) c_behind (a = target_rgba[3], blended before quantisation) and
 *   seg / depth report the target.  Body alpha is ignored (bodies are opaque).
 *   Shading: c = clamp(rgb (ambient + diffuse max(0, n . l)), 0, 1), n the unit normal turned to face the viewer, l the unit
 *   light_direction; byte = floor(255 c + 0.5).  Background colour where nothing is hit.
 *   Outputs (each may be NULL, not all three; each 16-byte aligned; nothing past its last byte is written):
 *     rgb   [num_envs][height][width][3] uint8 (the reference's np.array(rgb_pixels)[:, :, :3] per env)
 *     depth [num_envs][height][width] float32: eye depth along the view axis (render.project's depth), +inf where nothing is hit
 *     seg   [num_envs][height][width] uint8: enum pnr_seg
 * PNR_ERR_INVALID, no output touched, for: a null handle or params, a wrong struct_size, width or height outside 1..4096, fov_y
 * outside (0, 180), a near or far clip that is not finite and > 0, near_clip >= far_clip, a non-finite view or one whose 3x3 part
 * is not orthonormal, a non-finite or zero light_direction, non-finite ambient or diffuse, n_bodies outside 0..PNR_MAX_SCENE, a
 * bad shape or non-finite / degenerate body data (as pnr_config.scene), misaligned pointers, all outputs NULL, more than 2^31 - 1
 * tiles of 256 to 1 024 pixels, and a call before the first pnr_reset or pnr_set_state (the target comes from the state).
 * float32 arithmetic.  Parity unpinned: Bullet's TinyRenderer / OpenGL pixels are not reproduced (no shadows, textures or
 * anti-aliasing; the shading rule above is the engine's own).
 *
 * pnr_render_bodies is pnr_render with a world of its own per env: body_positions, with pnr_get_contacts' layout and meaning
 * ([num_envs][n_bodies][3] float32, 4-byte aligned, read only, or NULL): row [k][b] replaces bodies[b].position in env k;
 * orientation, size and colour stay shared; for a plane it is the point the plane passes through; ignored when n_bodies == 0.
 * Checks and refusals are pnr_render's (its messages name pnr_render), plus the alignment of body_positions.  With
 * body_positions == NULL it is pnr_render, byte for byte.
 * The moving sphere (a handle with PNR_BODY_IN_RENDER set, pnr_set_body_queries), in both calls: every env whose mass word is > 0
 * shows one more opaque sphere of the env's radius at the env's centre, in the colour pnr_set_body_queries holds, labelled
 * PNR_SEG_MOVING_BODY and shaded and depth-tested like a body.  Without per-env positions and without a shown sphere both calls
 * launch the kernel pnr_render always launched.
 */
enum pnr_seg {
    PNR_SEG_BACKGROUND = 0,
    PNR_SEG_LINK0 = 1,       /* + link_index: the URDF link of the visual (2 .. 11: robot:rotator1 .. robot:pointer) */
    PNR_SEG_TARGET = 12,
    PNR_SEG_BODY0 = 13,      /* + body index (13 .. 20) */
    PNR_SEG_MOVING_BODY = 21 /* the env's moving sphere: PNR_SEG_BODY0 + PNR_MAX_SCENE */
};
typedef struct pnr_render_params {
    uint32_t struct_size;              /* sizeof(pnr_render_params) */
    int32_t  width, height;            /* 1 .. 4096 each */
    int32_t  n_bodies;                 /* 0 .. PNR_MAX_SCENE */
    double   view[16];                 /* world -> eye, row-major 4x4 (render.view_matrix): eye looks along -z, +y up */
    double   fov_y, near_clip, far_clip;   /* RenderConfig.projection_fov (degrees), projection_near / far */
    double   light_direction[3];       /* towards the light, world frame (need not be unit) */
    double   ambient, diffuse;
    float    background[3];            /* rgb in [0, 1] */
    float    target_rgba[4];           /* PioneerKinematicConfig.target_rgba */
    int32_t  reserved;
    pnr_scene_body bodies[PNR_MAX_SCENE];  /* shape, position, orientation, size as in pnr_config.scene */
    float    body_rgba[PNR_MAX_SCENE][4];  /* rgb used, alpha ignored */
} pnr_render_params;
int pnr_render(pnr_handle h, const float* joint_state, const pnr_render_params* p, uint8_t* rgb, float* depth, uint8_t* seg,
               void* stream);
int pnr_render_bodies(pnr_handle h, const float* joint_state, const pnr_render_params* p, const float* body_positions, uint8_t* rgb,
                      float* depth, uint8_t* seg, void* stream);

/*
 * pnr_render_bodies through a camera of its own per env, one launch: getCameraImage with a view matrix computed per env, from
 * getLinkState for a camera on the arm (bullet_env.py:156-185 -> getCameraImage; bullet_scene.py:53-59 -> getLinkState).
 *   cameras      device float32 [7] (cameras_per_env = 0: one row for all envs) or [num_envs][7] (cameras_per_env = 1), 4-byte
 *                aligned, read only.  A row is position[3] | quaternion (x, y, z, w): the camera frame expressed in the parent
 *                frame.  The camera's axes are x right, y up, z towards the viewer; it looks along -z, the convention of
 *                p->view.  The kernel normalises the quaternion.  NULL: the camera pose is the inverse of p->view, which is then
 *                the transform parent frame -> eye frame (cameras_per_env is still checked).  With a non-NULL cameras p->view is
 *                not read.
 *   camera_link  the parent frame: -1 the world; 0 .. 10 that URDF link's frame of EACH env (pnr_get_link_states' link index;
 *                link 0 is the base, the world frame; link 10, robot:pointer, carries the fixed effector_to_pointer offset, as
 *                pnr_ray_test's parent_link does): an eye-in-hand camera.  The link's pose comes from the joints the arm is
 *                drawn from: joint_state, else the handle's own (dynamics mode the simulated q, kinematic mode the env's r).
 * Everything else is pnr_render_bodies': fov_y, near_clip, far_clip, the light (world frame), the hit rule, shading, labels,
 * the outputs, body_positions and the moving sphere where the handle shows it.  A camera inside a shape sees that shape's far
 * face (the hit rule's leaving candidate), so a wrist camera sits outside its link's shapes: on the pointer, whose sphere has
 * radius 0.2 about the link's origin, at a distance > 0.2 + near_clip from it, or it looks at the inside of that sphere.
 * Unlike Bullet's getCameraImage, depth is the eye depth along the view axis, not the depth buffer's value in [0, 1].
 * PNR_ERR_INVALID, nothing launched and no output touched, for: everything pnr_render_bodies refuses (p->view where it is
 * read: with cameras == NULL), camera_link outside -1..10, cameras_per_env outside {0, 1}, a cameras pointer that is not
 * 4-byte aligned.  The camera rows are device data and are not checked: a non-finite row or a zero quaternion may give THAT env
 * any bytes, inside that env's own spans of the outputs; nothing else is written and no other env changes.  An env's image does
 * not depend on the batch around it, bit for bit.  With camera_link == -1 and cameras == NULL the call is pnr_render_bodies: the
 * same launch, the same bytes.  float32 arithmetic: the camera, every shape's record and its pixel rectangle are built per env
 * on the device, where pnr_render builds the shared camera's static bodies on the host in double.
 */
int pnr_render_cameras(pnr_handle h, const float* joint_state, const pnr_render_params* p, const float* body_positions,
                       int32_t camera_link, const float* cameras, int32_t cameras_per_env, uint8_t* rgb, float* depth,
                       uint8_t* seg, void* stream);

/*
 * rayTest / rayTestBatch for every env, one launch: n_rays segments per env against that env's solids.
 *   Ray r is the segment from + t (to - from), t in [0, 1]: rays[...][0:3] is `from`, [3:6] is `to`, float32, 4-byte aligned,
 *   read only.  rays_per_env = 0: rays is [n_rays][6], shared by all envs; 1: [num_envs][n_rays][6].  parent_link = -1: the
 *   rays are in the world frame; 0 .. 10: in the frame of that URDF link of EACH env (pnr_get_link_states' link index,
 *   PyBullet's parentLinkIndex; link 0 is the base, the world frame): a sensor mounted on the arm.
 *   joint_state     as pnr_get_link_states ([num_envs][12] q | qd, 16-byte aligned, read only); NULL = the handle's own joints
 *                   (dynamics mode the simulated q, kinematic mode the env's r)
 *   body_positions  as pnr_get_contacts: [num_envs][n_bodies][3] float32 or NULL, a world position per env in place of
 *                   bodies[b].position.  Ignored when n_bodies == 0.
 *   Solids, selected by hit_mask (every shape is a solid):
 *     PNR_RAY_HIT_BODIES  bodies[] (as pnr_contact_params.bodies); a plane is the half-space below its surface
 *     PNR_RAY_HIT_ARM     the URDF's 14 <visual> shapes posed by the env's joints: pnr_render's primitives, so a ray and a
 *                         pixel see the same arm
 *     PNR_RAY_HIT_TARGET  a sphere of pnr_config.target_radius at the env's target (pnr_get_state words 18-20), opaque here
 *   Hit rule: a ray hits a solid at its entering parameter t_n if it starts outside the solid and 0 <= t_n <= 1.  A ray that
 *   starts inside a solid does not hit that solid (Bullet's rule for convex shapes; it makes a sensor inside the pointer's
 *   sphere usable).  The smallest t_n over the enabled solids wins; on a tie the order is arm visuals in table order, then the
 *   target, then bodies by index.  A zero-length ray misses.
 *   The moving sphere (a handle with PNR_BODY_IN_RAYS set, pnr_set_body_queries): where hit_mask has PNR_RAY_HIT_BODIES, every env
 *   whose mass word is > 0 has one more solid, a sphere of the env's radius at the env's centre, under the same rule (the
 *   entering parameter counts; a ray that starts inside does not hit it), label PNR_SEG_MOVING_BODY (21), after the caller's
 *   bodies on a tie.  hit_mask keeps its three bits.
 *   Outputs (at least one non-NULL, each 16-byte aligned; nothing past the last row is written):
 *     hits      [num_envs][n_rays][PNR_RAY_DIM] float32:
 *                 [0]   hit fraction t_n; 1 on a miss (PyBullet's convention)
 *                 [1:4] world hit position; `to` in the world frame on a miss
 *                 [4:7] unit outward world normal; 0 on a miss
 *                 [7]   the enum pnr_seg label as a float: 0 miss, 1 + link, 12 the target, 13 + body, 21 the moving sphere
 *     fractions [num_envs][n_rays] float32: [0] alone (the tensor that goes into an observation)
 * PNR_ERR_INVALID, nothing launched and no output touched, for: a null handle or params, a wrong struct_size, n_rays outside
 * 1..PNR_MAX_RAYS, parent_link outside -1..10, n_bodies outside 0..PNR_MAX_SCENE, a hit_mask that is 0 or has unknown bits,
 * rays_per_env not 0 or 1, NULL rays, both outputs NULL, misaligned pointers, a bad shape or non-finite / degenerate body data (as
 * pnr_get_contacts), a NULL joint_state or PNR_RAY_HIT_TARGET before the first pnr_reset (or pnr_set_state).  With a caller's
 * joint_state and no TARGET bit a fresh handle is accepted: nothing of the state is read.  Non-finite rays or joints give
 * non-finite or missing hits, unchecked.  An env's results do not depend on the batch around it, bit for bit.  float32
 * arithmetic, asynchronous on `stream`, no allocation, no synchronisation: capturable into a graph.  Parity unpinned: Bullet's
 * ray casts against its own collision shapes are not reproduced (the reference URDF has no <collision>, so Bullet itself would
 * hit the bodies only: the default mask).
 */
#define PNR_RAY_DIM 8
#define PNR_MAX_RAYS 1024                       /* per env */
enum pnr_ray_hit { PNR_RAY_HIT_BODIES = 1, PNR_RAY_HIT_ARM = 2, PNR_RAY_HIT_TARGET = 4 };
typedef struct pnr_ray_params {
    uint32_t struct_size;     /* sizeof(pnr_ray_params) */
    int32_t  n_rays;          /* 1 .. PNR_MAX_RAYS rays per env */
    int32_t  rays_per_env;    /* 0: rays is [n_rays][6], shared by all envs; 1: [num_envs][n_rays][6] */
    int32_t  parent_link;     /* -1: rays are in the world frame; 0 .. 10: in that URDF link's frame of EACH env */
    int32_t  hit_mask;        /* pnr_ray_hit bits, non-zero; default PNR_RAY_HIT_BODIES */
    int32_t  n_bodies;        /* 0 .. PNR_MAX_SCENE */
    pnr_scene_body bodies[PNR_MAX_SCENE];       /* as pnr_contact_params.bodies */
} pnr_ray_params;
int pnr_ray_params_default(pnr_ray_params* p);
int pnr_ray_test(pnr_handle h, const float* joint_state, const pnr_ray_params* p, const float* rays,
                 const float* body_positions, float* hits, float* fractions, void* stream);

/* Diagnostic: the engine's float32 sin/cos (the np.sin/np.cos replacement used
 * for obs entries, pioneer_knm_env.py:195-203) over a device array x[n].
 * bounded != 0 selects the Cody-Waite path used for r, v and limit distances;
 * 0 the path used for raw actions (falls back to full reduction above 2^17). */
int pnr_diag_sincos(const float* x, float* sin_out, float* cos_out, int64_t n,
                    int bounded, void* stream);

/* Host-driver helper (not part of the env surface): the element-wise part of the PPO loss with the
 * hyper-parameters of pioneer/launch/pioneer_knm_train.py:45-67 (clip_param, vf_clip_param,
 * vf_loss_coeff; kl_coeff and entropy_coeff as device scalars because they change between captured
 * replays), forward and backward in one launch.  head_policy / head_value are the two nets' raw
 * outputs as rows of 16 floats (means 0..5, log-stds 6..11 | value 0); the gradients of the batch-mean
 * loss come back in the same layout; partial_sums [partial_rows][8] receives per-block sums of
 * (policy_loss, vf_loss, kl, entropy, total) with partial_rows >= ceil(batch / 256).  idx (int64 [batch], or NULL) is
 * the minibatch gather: sample i's rollout record (actions .. value_old) is row idx[i] of those arrays, while the
 * head rows and their gradients are indexed by i.  means (8 floats, or NULL) receives the five batch means, summed from
 * partial_sums in row order by a second small launch.  Device pointers. */
int pnr_ppo_loss(int64_t batch, const int64_t* idx, const float* head_policy, const float* head_value, const float* actions,
                 const float* logp_old, const float* mean_old, const float* log_std_old, const float* adv,
                 const float* value_target, const float* value_old, const float* kl_coeff,
                 const float* entropy_coeff, float clip_param, float vf_clip_param, float vf_loss_coeff,
                 float* grad_head_policy, float* grad_head_value, float* partial_sums, int64_t partial_rows,
                 float* means, void* stream);

/*
 * Host-driver helper: after the sampler's T steps, one launch for the log-probabilities of the taken actions (diagonal
 * Gaussian, actions / mean / log_std [T][n][6]; pass actions NULL to skip) and GAE(lambda) advantages and value targets
 * [T][n] from reward / values [T][n], last_value [n] (the bootstrap value) and the done / truncated bytes of pnr_step
 * (terminal = done | truncated, as RLlib 0.8's postprocessing treats the TimeLimit cut; truncated may be NULL).
 * terminals [T][n] (1.0 / 0.0) is optional.  gamma / lambda: the reference leaves RLlib's defaults (0.99 / 1.0).
 * stats (optional): the rollout's bookkeeping in the same launch — the episode statistics behind the reference's result
 * columns episode_reward_{max,min,mean} / episode_len_mean (cli.py:32-38): ep_ret / ep_len [n] are each env's running return
 * and length (in / out, carried across rollouts), w_sum / w_len / w_cnt (float64) and w_max / w_min (float32) the window
 * accumulators of the episodes that ended, updated in place; adv_stats [3] (float64) receives the advantages' sum, sum of
 * squares and count (PPO standardises them over the global batch).  scratch: pnr_ppo_gae_scratch(n) doubles.
 */
typedef struct pnr_rollout_stats {
    float* ep_ret; float* ep_len;
    double* scratch; int64_t scratch_doubles;
    double* w_sum; double* w_len; double* w_cnt; float* w_max; float* w_min;
    double* adv_stats;
} pnr_rollout_stats;
int64_t pnr_ppo_gae_scratch(int64_t n);
int pnr_ppo_gae(int32_t T, int64_t n, const float* reward, const float* values, const float* last_value, const uint8_t* done,
                const uint8_t* truncated, const float* actions, const float* mean, const float* log_std, double gamma,
                double lambda, float* logp, float* adv, float* value_target, float* terminals, const pnr_rollout_stats* stats,
                void* stream);

/*
 * Host-driver helper: the moment pass of the observation filter ('observation_filter': 'ConcurrentMeanStdFilter',
 * pioneer_knm_train.py:66) over obs [rows][137]: dsum[c] += sum_r (obs[r][c] - pivot[c]), dsq[c] += sum_r (...)^2 (float64
 * accumulators [137]; float32 partial sums over 512 rows each, added in order), *dn += rows; one read of the buffer.
 * scratch: pnr_filter_moments_scratch(rows) floats.
 */
int64_t pnr_filter_moments_scratch(int64_t rows);
int pnr_filter_moments(int64_t rows, const float* obs, const float* pivot, float* scratch, int64_t scratch_floats, double* dsum,
                       double* dsq, double* dn, void* stream);

/* The filter's merge on one rank (MeanStdFilter.sync): the pending delta *dn, dsum / dsq [137] (zeroed on return) about
 * pivot [137] into the running *n, mean / m2 [137] by Chan's update, float64, one launch. */
int pnr_filter_merge(double* dn, double* dsum, double* dsq, const float* pivot, double* n, double* mean, double* m2, void* stream);

/* MeanStdFilter.prepare() in one launch ('observation_filter': 'ConcurrentMeanStdFilter', pioneer_knm_train.py:66): the float32 vectors
 * the kernels filter with, x' = clamp((x - loc) * inv, lo, hi), from the
 * running statistics *n, mean / m2 [137] (RLlib MeanStdFilter: (x - mean) / (std + 1e-8), clipped to +-clip; clip = +inf: no clipping;
 * the identity until two samples exist). */
int pnr_filter_prepare(const double* n, const double* mean, const double* m2, double clip, float* loc, float* inv, float* lo, float* hi,
                       void* stream);

/*
 * Host-driver helper: out[0..n) = a pseudo-random permutation of 0..n-1 keyed by (seed, stream_id) — a Feistel network
 * with cycle walking, one launch and no sort; the SGD epochs' minibatch shuffle (RLlib sgd.py shuffles each epoch).
 */
int pnr_permutation(int64_t n, uint64_t seed, uint64_t stream_id, int64_t* out, void* stream);

/*
 * Host-driver helpers (not part of the env surface): the two MLPs of the reference's PPO config — 'fcnet_hiddens':
 * [256, 256] (pioneer/launch/pioneer_knm_train.py:59-61), tanh, separate policy (12 outputs: 6 means + 6 log-stds) and
 * value (1 output) nets, RLlib's FullyConnectedNetwork with vf_share_layers False — as bf16 MFMA kernels.
 *   params / grads  12 device pointers, net-major: policy w1 [256][137], b1 [256], w2 [256][256], b2 [256],
 *                   w3 [n3][256], b3 [n3], then the value net's six; float32, row-major [out][in] as the host keeps them
 *   wpack           pnr_mlp_pack_elems() bf16 values; bias: pnr_mlp_bias_elems() floats (written by pnr_mlp_pack)
 *   obs             [rows][137] float32; idx [batch] int64 row gather or NULL; f_loc/f_inv/f_lo/f_hi [137] or all NULL:
 *                   the nets see clamp((obs - loc) * inv, lo, hi), the MeanStdFilter of the reference's config (:66)
 *   head            [2][batch][16] float32: policy rows = means 0..5, raw log-stds 6..11; value rows = v at column 0
 *   xs [batch][144], h1 / h2 / dz1 / dz2 [2][batch][256] bf16: activations kept for / made by the backward pass
 *   slabs           >= pnr_mlp_slab_floats(batch) floats of scratch (per-slice partial gradients, summed in order)
 * pnr_mlp_backward = backward-data + weight gradients + reduction; gradients of the batch as given by g_head
 * [2][batch][16] (d loss / d head), times the device scalar *scale when scale != NULL, written (accumulate = 0) or
 * added (1) to `grads`.
 */
int64_t pnr_mlp_pack_elems(void);
int64_t pnr_mlp_bias_elems(void);
int64_t pnr_mlp_slab_floats(int64_t batch);
/*
 * `planes` (1, 2 or 3) selects the precision of every MFMA operand of the pnr_mlp_* kernels; accumulation is float32 always.
 *   1: bf16 operands (8 significant bits) — the reduced-precision fast variant.
 *   2: each float32 operand as TWO FP16 PLANES (ABI 5): p0 = fp16(s x), p1 = fp16(s x - p0) with a power-of-two scale s per tensor
 *      (weights 2^8, activations 2^8, net inputs 2^4, gradients 4 * 2^ceil(log2 batch); the accumulators are divided by the product
 *      of the two scales, exactly) — 22 significant bits per operand, the three fp16 MFMAs (0,0), (0,1), (1,0) per product.  Measured
 *      at a float32 framework GEMM's own distance from float64 (heads 2.9e-7 against 3.8e-7; gradients 9.6e-7 against 2.4e-6 of float32
 *      autograd): the accuracy of a float32 GEMM, i.e. what the reference's float32 learner computes in (pioneer_knm_train.py:47).
 *      Range: scaled values are clamped to +-65504 — weights |w| < 255, inputs |x| < 4094, per-sample gradients |dL/dz| < 16 384.
 *   3: three bf16 planes (24 bits, exact split, no range caveat), the six bf16 MFMAs of the plane pairs i + j < 3 per product (ABI 4).
 * Every 16-bit operand buffer then exists `planes` times, plane-major: wpack [planes][pnr_mlp_pack_elems()], xs / xs_out / xs_in
 * [planes][batch][144], h1 / h2 / dz1 / dz2 [planes][2][batch][256].  Biases, heads, slabs, Adam state and master weights are float32 either way.
 * planes > 1: pnr_mlp_forward / pnr_mlp_act save no activations (xs, h1, h2 / xs_out must be NULL: pnr_mlp_backward is bf16-only and
 * the learner gathers its inputs from the float32 observations), pnr_mlp_gather takes no xs_rows, pnr_mlp_train_step needs w3_partials.
 */
int pnr_mlp_pack(const float* const* params, int32_t n3_policy, int32_t n3_value, void* wpack, float* bias, int32_t planes, void* stream);
int pnr_mlp_forward(int64_t batch, const float* obs, const int64_t* idx, const float* f_loc, const float* f_inv,
                    const float* f_lo, const float* f_hi, const void* wpack, const float* bias, float* head,
                    void* xs, void* h1, void* h2, int32_t first_net, int32_t n_nets, int32_t planes, void* stream);
/*
 * The sampler's per-step launch: both nets forward on `obs` [batch][137] and, in the policy net's last epilogue, the
 * action draw of RLlib's DiagGaussian (what the reference's PPO config samples with): log_std = clamp(raw, -20, 2),
 * actions = mean + exp(log_std) * noise (noise [batch][6] standard-normal draws supplied by the caller), env_actions =
 * clamp(actions, -a_max, a_max) (a_max [6]; the env's action space, pioneer_knm_env.py:60-61; NULL: no clipping and
 * env_actions is not written).  mean / log_std / actions / env_actions [batch][6], values [batch]; head [2][batch][16] or NULL;
 * xs_out [batch][144] bf16 or NULL: the nets' input as they saw it (filtered, rounded), which the learner's epoch gather
 * (pnr_mlp_gather's xs_rows) copies instead of re-making it from the float32 observations.
 */
int pnr_mlp_act(int64_t batch, const float* obs, const float* f_loc, const float* f_inv, const float* f_lo, const float* f_hi,
                const void* wpack, const float* bias, const float* noise, const float* a_max, float* head, float* mean,
                float* log_std, float* values, float* actions, float* env_actions, void* xs_out, int32_t planes, void* stream);
/*
 * The sampler's closed loop as ONE resident launch: T x (pnr_mlp_act, pnr_step) for every env of handle `h` — per step both nets
 * on the observation in slot t of `obs`, the DiagGaussian draw and clip as in pnr_mlp_act, then BulletEnv.step
 * (bullet_env.py:192-197) with that action: reward / done / truncated [T][n] and the next observation into slot t + 1.  A
 * workgroup owns 64 envs for all T steps (env state, observation tile and both nets' W2 stay on the CU).  Replaces the RLlib
 * rollout worker's act -> env.step loop (the reference: one env per worker process, pioneer_knm_train.py:49) for kinematic-mode
 * handles with env-major layouts; results equal the per-step calls bit for bit.
 *   obs [T + 1][n][137]: slot 0 = where the rollout starts (what the last pnr_step / pnr_reset / rollout left), slots 1..T written
 *   noise [T][n][6] standard-normal draws; a_max [6] or NULL (no clipping); f_loc..f_hi [137] each or all NULL
 *   mean / log_std / actions [T][n][6] (8-byte aligned), values [T][n], xs_out [T][n][144] bf16 or NULL
 */
int pnr_ppo_rollout(pnr_handle h, int32_t T, const float* f_loc, const float* f_inv, const float* f_lo, const float* f_hi,
                    const void* wpack, const float* bias, const float* noise, const float* a_max, float* obs, float* mean,
                    float* log_std, float* values, float* actions, void* xs_out, float* reward, uint8_t* done, uint8_t* truncated,
                    void* stream);
int pnr_mlp_backward(int64_t batch, const float* g_head, const void* wpack, const void* xs, const void* h1, const void* h2,
                     void* dz1, void* dz2, float* slabs, int64_t slab_floats, float* const* grads, int32_t n3_policy,
                     int32_t n3_value, int32_t accumulate, const float* scale, void* stream);

/*
 * One PPO minibatch update of both nets in three launches, nothing of it on the host: (1) per 64-sample tile and net the
 * forward pass (activations saved for the weight gradients), the tile's share of the loss and its backward-data pass in
 * ONE kernel (which also counts the update in *adam_step); (2) weight gradients per batch slice; (3) EITHER the fused
 * slab-reduction + Adam + bf16 repacking, one extra block of which sums the loss means (flat_grad == NULL), OR the
 * loss means in a small launch of their own and the reduction into flat_grad
 * [pnr_mlp_grad_floats()] with no update: a multi-GPU run all-reduces that bucket and calls pnr_mlp_adam(s, flat_grad,
 * 1 / world_size, stream).  The update is Adam with the arithmetic of the optimiser the reference trains with ('lr' of its
 * config, pioneer_knm_train.py:64; betas 0.9 / 0.999, eps 1e-8; no weight decay) with its state m, v kept as
 * [pnr_mlp_grad_floats()] floats each.  wpack / bias must hold the CURRENT weights on entry (pnr_mlp_pack once, then
 * every update refreshes them).  All pointers are device pointers; `means` receives (policy_loss, vf_loss, kl,
 * entropy, total, 0, 0, 0).  partials: scratch of partial_rows >= 2 * ceil(batch / 64) rows of 8 floats; `head` is not
 * written (the head rows never leave the chip); g_head [2][batch][16] is written ONLY when w3_partials is NULL (with
 * w3_partials nothing outside the tile reads the head gradients, they stay on the chip, g_head is left as it was and may be
 * NULL).  wpack, bias, adam_m, adam_v, slabs and flat_grad must be 16-byte aligned (PNR_ERR_INVALID otherwise: the optimiser
 * kernel moves them four floats at a time); so must xs_in, and with planes > 1 xs_in_plane must be 0 or a multiple of 8
 * elements >= batch * 144 (the kernels read 16-byte vectors at xs_in + plane * xs_in_plane).  Every argument is checked
 * before the first launch: an error return has launched nothing and counted no update.
 */
typedef struct pnr_mlp_step {
    uint32_t struct_size;   /* sizeof(pnr_mlp_step) */
    int64_t batch;
    const float* obs; const int64_t* idx;
    const float* f_loc; const float* f_inv; const float* f_lo; const float* f_hi;
    const float* actions; const float* logp_old; const float* mean_old; const float* log_std_old;
    const float* adv; const float* value_target; const float* value_old;
    const float* kl_coeff; const float* entropy_coeff;
    float clip_param, vf_clip_param, vf_loss_coeff;
    float* params[12]; int32_t n3_policy, n3_value;
    void* wpack; float* bias;
    float* adam_m; float* adam_v; float* adam_step;
    float lr, beta1, beta2, eps;
    float* head; float* g_head; void* xs; void* h1; void* h2; void* dz1; void* dz2;
    float* partials; int64_t partial_rows; float* slabs; int64_t slab_floats;
    float* means;
    float* flat_grad;
    const void* xs_in;      /* optional [batch][144] bf16: the nets' input already gathered, filtered and rounded by
                             * pnr_mlp_gather.  Then obs / idx / the filter vectors are not read, the record arrays (actions ..
                             * value_old) are read row by row, and `xs` is not written */
    int32_t first_net, n_nets; /* the nets this call works on: 0, 0 (or 0, 2) = both; 0, 1 = the policy net; 1, 1 = the value net.
                             * The two nets share nothing but their input (vf_share_layers False), so a multi-GPU run may drive them
                             * as two independent chains on two streams — each train_step -> all-reduce of ITS half of flat_grad
                             * -> pnr_mlp_adam — and one net's all-reduce overlaps the other's kernels.  Every call counts one update
                             * in *adam_step: two chains need two counters.  `means` of a one-net call holds that net's terms only
                             * (policy: policy_loss, kl, entropy and their share of total; value: vf_loss and its share): the
                             * update's means are the element-wise sum of the two rows.  partial_rows >= n_nets * ceil(batch / 64) */
    float* w3_partials;     /* optional scratch, w3_partial_floats >= pnr_mlp_w3_partial_floats(batch): the fused kernel then leaves layer 3's */
    int64_t w3_partial_floats; /* weight-gradient products per 64-sample tile there (17 KB) instead of storing H2 (32 KB per tile) for the
                             * weight-gradient kernel, which adds them in tile order: the same sums bit for bit, 30 % fewer bytes in that
                             * kernel.  NULL: H2 is stored to h2 and read back (h2 must be given either way) */
    int32_t planes;         /* 0 or 1: bf16 operands; 2, 3: split float32 operands (see pnr_mlp_pack): wpack, xs_in / xs, h1, dz1, dz2 hold
                             * `planes` planes, w3_partials must be given, Adam refreshes every plane of wpack */
    int64_t xs_in_plane;    /* planes > 1: elements between two planes of xs_in; 0 = batch * 144.  (A minibatch inside an epoch's
                             * gathered planes [planes][rows][144]: xs_in = plane 0's first row of it, xs_in_plane = rows * 144) */
} pnr_mlp_step;
int64_t pnr_mlp_w3_partial_floats(int64_t batch);
/*
 * An SGD epoch's shuffle applied once: row i of every output is row idx[i] of the corresponding input — the observation
 * filtered and rounded to the nets' input layout (xs_out [batch][144] bf16) and the rollout record — so that the epoch's
 * minibatch updates read contiguous rows (pnr_mlp_step.xs_in = xs_out + 144 * first_row, record pointers likewise).
 * record_rows (optional): the same record as ONE row of 24 floats per sample, made once per iteration by
 * pnr_ppo_pack_record (actions 0..5 | mean 6..11 | log_std 12..17 | logp, adv, value_target, value_old | 2 pad; adv
 * standardised as (adv - *adv_mu) / *adv_den when the two device scalars are given): the gather then reads one or two cache
 * lines per sample for the record instead of seven, and the seven input arrays may be NULL.  xs_rows (optional, [rows][144]
 * bf16): the net inputs saved by pnr_mlp_act; then obs and the filter vectors are not read (288-byte rows instead of 548).
 */
int pnr_ppo_pack_record(int64_t rows, const float* actions, const float* logp_old, const float* mean_old, const float* log_std_old,
                        const float* adv, const float* value_target, const float* value_old, const float* adv_mu, const float* adv_den,
                        float* record_rows, void* stream);
int pnr_mlp_gather(int64_t batch, const int64_t* idx, const float* obs, const float* f_loc, const float* f_inv, const float* f_lo,
                   const float* f_hi, const float* actions, const float* logp_old, const float* mean_old, const float* log_std_old,
                   const float* adv, const float* value_target, const float* value_old, void* xs_out, float* actions_out,
                   float* logp_out, float* mean_out, float* log_std_out, float* adv_out, float* value_target_out,
                   float* value_old_out, const float* record_rows, const void* xs_rows, int32_t planes, void* stream);
int64_t pnr_mlp_grad_floats(void);
int pnr_mlp_train_step(const pnr_mlp_step* s, void* stream);
int pnr_mlp_adam(const pnr_mlp_step* s, const float* flat_grad, float grad_scale, void* stream);

int64_t pnr_num_envs(pnr_handle h);

/* Last error message of `h`, or of the calling thread when h == NULL. */
const char* pnr_last_error(pnr_handle h);

int pnr_abi_version(void);

/* What this binary was built from: "api=<sha16>;learn=<sha16>;" — per translation unit, the first 16 hex digits of sha256 over
 * the compile flags, the unit's source files and this header, baked in at compile time (-DPNR_UNIT_FINGERPRINT).  The Python
 * loader (pioneer_amd/_lib.py load_library) recomputes it from the tree and refuses a library that differs; bench.py prints
 * it next to the fingerprints of the committed counter passes.  (No reference counterpart: build hygiene.) */
const char* pnr_build_fingerprint(void);

#ifdef __cplusplus
}
#endif
#endif /* PIONEER_AMD_H */
