"""The inputs of the inverse-dynamics tests, shared by the CPU tests (which measure on them what float32 arithmetic alone costs
and assert the conditions the bars rest on) and the GPU tests (which run the kernels on exactly these inputs).  Nothing here is
a reference: that is tests/inverse_dynamics_ref.py.

Inputs: q uniform in +-0.9 x the joint limits, qd in +-3, qdd in +-20, each from a generator of its own, so the inputs of n envs
are the first n rows of the inputs of N_MAX envs and what is measured at N_MAX covers every smaller batch.  All values are float32
numbers (the engine's input format), held in float64 where a reference reads them.

THE FLOAT32 FLOOR.  inverse_dynamics_ref.newton_euler runs the same Newton-Euler arithmetic in float32 and in float64 on the same
float32 inputs; the per-joint largest difference over the batch is what float32 alone costs on these inputs, whatever the order of
operations.  TAU_FLOOR / M_FLOOR are those maxima, measured with tests/test_inverse_dynamics_cpu.py::
test_float32_floor_constants_hold_on_the_inputs (numpy 2.x, x86-64; N_MAX envs; gravity 0 and 9.81; unit link scales, drawn link
scales, and the drawn-scale envs after two free-falling world steps; with and without the joint losses), rounded up to two
digits:
    tau, per joint:   1.1e-2  1.9e-2  1.3e-2  2.3e-3  1.6e-3  7.8e-4
                      (measured 1.005e-2 1.870e-2 1.286e-2 2.231e-3 1.516e-3 7.759e-4; the smallest batch medians of |tau_i|
                      over those cases are 1.1e3 1.8e3 1.1e3 9.0e1 1.5e2 7.4e1, so every constant is <= 2e-5 of its median)
    M, per entry:     M_FLOOR below, the larger of (i, j) and (j, i); largest 9.0e-4 at (1, 1), where M reaches 2.8e3
The kernels are allowed FLOOR_MARGIN = 8 times these: for their different order of operations (body-frame recursions, fused
multiply-adds, packed pairs) and for sincos_any's error against libm.
"""
import numpy as np

import ik_ref
import inverse_dynamics_ref as ref
import oracle_cases as ocases
import world_step_ref as wref
from oracle import DynOracle

DOF = 6
N_MAX = 1000
SEED = 21
GRAVITIES = (0.0, 9.81)
H = 1.0 / 240
STEP_TIME = 10 * H
FLOOR_MARGIN = 8.0

# measured: see the module docstring; test_float32_floor_constants_hold_on_the_inputs asserts floor <= constant <= 2 floor
TAU_FLOOR = np.array([1.1e-02, 1.9e-02, 1.3e-02, 2.3e-03, 1.6e-03, 7.8e-04])
M_FLOOR = np.array([
    [6.2e-04, 1.2e-04, 7.4e-05, 9.1e-05, 5.2e-05, 2.7e-05],
    [1.2e-04, 9.0e-04, 4.2e-04, 1.2e-04, 4.6e-05, 3.3e-05],
    [7.4e-05, 4.2e-04, 3.1e-04, 6.6e-05, 3.4e-05, 2.7e-05],
    [9.1e-05, 1.2e-04, 6.6e-05, 1.5e-05, 8.1e-06, 6.1e-06],
    [5.2e-05, 4.6e-05, 3.4e-05, 8.1e-06, 1.4e-05, 7.7e-06],
    [2.7e-05, 3.3e-05, 2.7e-05, 6.1e-06, 7.7e-06, 5.0e-06],
])


def joints(n, frac=0.9, qd_max=3.0, qdd_max=20.0, seed=SEED):
    """q, qd, qdd [n, 6] as float32 arrays"""
    lo, hi = (v.astype(np.float64) for v in ik_ref.limits_f32())
    q = np.random.default_rng(seed).uniform(frac * lo, frac * hi, size=(n, DOF))
    qd = np.random.default_rng(seed + 1).uniform(-qd_max, qd_max, size=(n, DOF))
    qdd = np.random.default_rng(seed + 2).uniform(-qdd_max, qdd_max, size=(n, DOF))
    return q.astype(np.float32), qd.astype(np.float32), qdd.astype(np.float32)


def make_oracle(n, gravity, randomize, seed=SEED, **dyn):
    """A reset oracle batch: unit link scales and the configured losses, or the per-env draws of `seed` (the engine's own)."""
    return ocases.make_oracle(seed, n, 10, gravity, dict(dyn, randomize=randomize))


def free_joints(orc):
    """every joint on zero gains: no motor torque at all (the PD law)"""
    for j in range(DOF):
        orc.set_joint_motor(j, 1, target_velocity=0.0, velocity_gain=0.0, max_force=0.0, max_velocity=0.0)


FREE_MOTORS = [dict(kind="pd", control_mode=1, target_velocity=0.0, position_gain=0.0, velocity_gain=0.0, max_force=0.0)] * DOF


def losses32(qd, friction, damping):
    qd, friction, damping = (np.asarray(x, dtype=np.float32) for x in (qd, friction, damping))
    return damping * qd + friction * qd / np.sqrt(qd * qd + np.float32(wref.FRICTION_EPS) ** 2)


def tau_floor(q, qd, qdd, scales, gravity, friction=None, damping=None):
    """[6]: per joint, the largest |float32 - float64| of the Newton-Euler torques over the batch (inputs: float32 numbers)"""
    f32 = lambda x: np.asarray(x, dtype=np.float32)  # noqa: E731
    t32 = ref.newton_euler(f32(q), f32(qd), f32(qdd), f32(scales), gravity, np.float32)
    t64 = ref.newton_euler(f32(q).astype(np.float64), f32(qd).astype(np.float64), f32(qdd).astype(np.float64),
                           f32(scales).astype(np.float64), gravity, np.float64)
    if friction is not None:
        t32 = t32 + losses32(qd, friction, damping)
        qd64 = f32(qd).astype(np.float64)
        t64 = t64 + f32(damping).astype(np.float64) * qd64 + f32(friction).astype(np.float64) * qd64 / np.sqrt(qd64 * qd64 + wref.FRICTION_EPS ** 2)
    return np.abs(t32.astype(np.float64) - t64).max(axis=0), np.median(np.abs(t64), axis=0)


def m_floor(q, scales):
    """[6, 6]: per entry, the largest |float32 - float64| of the Newton-Euler mass matrix over the batch"""
    q32, s32 = np.asarray(q, dtype=np.float32), np.asarray(scales, dtype=np.float32)
    M32 = ref.newton_euler_mass_matrix(q32, s32, np.float32)
    M64 = ref.newton_euler_mass_matrix(q32.astype(np.float64), s32.astype(np.float64), np.float64)
    return np.abs(M32.astype(np.float64) - M64).max(axis=0)


HOLD_SEED = 33                                                        # the gravity-hold scenario's link draws


def hold_poses(n, seed=31):
    """[n, 6] float32: |q_i| in 0.2 .. 0.8 x the joint's limit, random signs (poses an arm under gravity falls out of)"""
    lo, hi = ik_ref.limits_f32()
    rng = np.random.default_rng(seed)
    lim = np.minimum(np.abs(lo), np.abs(hi)).astype(np.float64)
    q = rng.uniform(0.2, 0.8, size=(n, DOF)) * lim * rng.choice([-1.0, 1.0], size=(n, DOF))
    return q.astype(np.float32)


# ---- the scenario of the torque world step against the reference: contacts, capped PD motors on joints 0-2, joints 3-5 free ----
BOX = dict(obstacle_position=(10.0, 5.0, 0.0), obstacle_half_extents=(0.5, 0.5, 5.0))
TORQUE_SCALE = np.array([20.0, 20.0, 20.0, 5.0, 5.0, 2.0])
PD_TARGETS, PD_FORCES, PD_KP, PD_KD = (0.4, -0.3, 0.5), (300.0, 600.0, 300.0), 4000.0, 400.0
TORQUE_MOTORS = [dict(kind="pd", control_mode=0, target_position=PD_TARGETS[j], target_velocity=0.0, position_gain=PD_KP,
                      velocity_gain=PD_KD, max_force=PD_FORCES[j], max_velocity=0.0) for j in range(3)] + FREE_MOTORS[3:]


def torque_scenario(n, seed=41):
    """q (+-0.6 x the limits), qd (+-1.5) and the external torques (+-TORQUE_SCALE) [n, 6], float32"""
    q, qd, _ = joints(n, frac=0.6, qd_max=1.5, seed=seed)
    tau = np.random.default_rng(seed + 3).uniform(-1.0, 1.0, size=(n, DOF)) * TORQUE_SCALE
    return q, qd, tau.astype(np.float32)


def torque_oracle(n):
    return DynOracle(n, dyn=dict(gravity=9.81, ground_z=0.0, link_contacts=1, **BOX))
