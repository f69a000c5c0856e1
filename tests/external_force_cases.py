"""The inputs of the external-force tests, shared by the CPU tests (which assert on the float64 reference that the inputs are well
conditioned and that the wrenches matter) and the GPU tests (which run the kernel on exactly these inputs).  Nothing here is a
reference: that is tests/world_step_ref.py with tests/external_force_ref.py.

Every input is a float32 number (the engine's input format), held in float64 where the reference reads it, and comes from a
generator of its own, so the inputs of n envs are the first n rows of the inputs of N_MAX envs: what the CPU tests establish on the
envs of `followed(N_MAX)` and the first 64 covers every batch size the GPU tests use.

The families (the issue's table).  PHYS is the kernel instantiation a family runs (bit 0 contacts, bit 1 the inertia-scaled motor):
    A   gravity, the env-wide PD motors on the command state; K = 1: a world force on the pointer, at the pointer        PHYS 0
    B   no gravity, no motors; K = 4: mixed frames on four links, forces, torques and off-origin points; randomised
        link masses, friction and damping                                                                               PHYS 0
    C   B with the ground plane and link contacts (a share of the envs touches it)                                      PHYS 1
    D   B's records under the inertia-scaled env-wide motors                                                            PHYS 2
    Dc  D with C's plane and link contacts: the fourth instantiation, which A-D alone would leave out                   PHYS 3
Sizes.  The forces are sized so that test_external_force_cpu.py's conditions hold (the wrench moves qd by more than 10 QD_TOL in
one world step, also when it acts in the first sub-step only against the motors' damping; rounding the inputs and the state to
float32 moves three world steps by less than a quarter of the bars).
"""
import numpy as np

import bars
import ik_ref
import oracle_cases as ocases

DOF = 6
N_MAX = 1000
SIZES = [1, 37, 64, 1000]
STEPS = 3
H = 1.0 / 240
FRAME_SKIP = 10
Q_TOL, QD_TOL = bars.Q_TOL, bars.QD_TOL                               # read through this module by tests/test_external_force_cpu.py

FREE = [dict(kind="pd", control_mode=1, target_velocity=0.0, position_gain=0.0, velocity_gain=0.0, max_force=0.0)] * DOF
TRACK = [None] * DOF                                                  # the env-wide law on the env's command state
MIXED = [(3, "link"), (5, "world"), (7, "link"), (10, "world")]       # arm1, rotator2, arm3, pointer
PLANE = dict(ground_z=0.0, link_contacts=True)
TORQUE_SCALE = np.array([20.0, 20.0, 20.0, 5.0, 5.0, 2.0])

FAMILIES = {
    "A": dict(seed=51, gravity=9.81, engine={}, motors=TRACK, specs=[(10, "world")], force=400.0, torque=0.0, offset=0.0, near=0.05, qd=0.5),
    "B": dict(seed=52, gravity=0.0, engine=dict(randomize=True), motors=FREE, specs=MIXED, force=30.0, torque=15.0, offset=1.0, frac=0.6, qd=1.0),
    "C": dict(seed=53, gravity=0.0, engine=dict(randomize=True, **PLANE), motors=FREE, specs=MIXED, force=30.0, torque=15.0, offset=1.0,
              frac=0.6, qd=1.0),
    "D": dict(seed=54, gravity=0.0, engine=dict(pd_inertia_scaled=True, pd_kp=400.0, pd_kd=40.0, torque_limit=2e4), motors=TRACK,
              specs=MIXED, force=400.0, torque=200.0, offset=1.0, near=0.05, qd=0.5),
    "Dc": dict(seed=55, gravity=0.0, engine=dict(pd_inertia_scaled=True, pd_kp=400.0, pd_kd=40.0, torque_limit=2e4, **PLANE), motors=TRACK,
               specs=MIXED, force=400.0, torque=200.0, offset=1.0, near=0.05, qd=0.5),
}
PHYS = {"A": 0, "B": 0, "C": 1, "D": 2, "Dc": 3}
HOLDS = (1, 4, 0)                                                     # Bullet's literal one sub-step, four of the ten, all of them


def followed(n):
    """The envs the reference follows: all of a small batch; of 1000, every 8th and the whole partial last wave."""
    return np.arange(n) if n <= 64 else np.array([e for e in range(n) if e % 8 == 0 or e >= (n // 64) * 64])


def make_oracle(family, n, reset=True):
    f = FAMILIES[family]
    return ocases.make_oracle(f["seed"], n, FRAME_SKIP, f["gravity"], f["engine"], reset=reset)


def states(family, r_cmd, rounded=True):
    """q, qd [n, 6] for the command positions r_cmd [n, 6] (the first n envs).  Motors that track the command state start `near`
    it (the PD law's pull stays moderate); free joints anywhere within frac x the limits."""
    f = FAMILIES[family]
    n = r_cmd.shape[0]
    lo, hi = (v.astype(np.float64) for v in ik_ref.limits_f32())
    rng = np.random.default_rng(f["seed"] + 100)
    if "near" in f:
        q = np.clip(r_cmd.astype(np.float64) + rng.uniform(-f["near"], f["near"], size=(N_MAX, DOF))[:n], 0.98 * lo, 0.98 * hi)
    else:
        q = rng.uniform(f["frac"] * lo, f["frac"] * hi, size=(N_MAX, DOF))[:n]
    qd = np.random.default_rng(f["seed"] + 101).uniform(-f["qd"], f["qd"], size=(N_MAX, DOF))[:n]
    return (q.astype(np.float32), qd.astype(np.float32)) if rounded else (q, qd)


def wrenches(family, q, rounded=True):
    """[n, K, 9] force | position | torque for the poses q [n, 6].  A world-frame record's point is the link origin's world
    position at q plus an offset; a link-frame record's point is the offset in the link's frame."""
    f = FAMILIES[family]
    n = q.shape[0]
    rng = np.random.default_rng(f["seed"] + 102)
    K = len(f["specs"])
    w = np.zeros((N_MAX, K, 9))
    w[:, :, 0:3] = rng.uniform(-f["force"], f["force"], size=(N_MAX, K, 3))
    w[:, :, 3:6] = rng.uniform(-f["offset"], f["offset"], size=(N_MAX, K, 3))
    w[:, :, 6:9] = rng.uniform(-f["torque"], f["torque"], size=(N_MAX, K, 3))
    w = w[:n]
    for j, (link, frame) in enumerate(f["specs"]):
        if frame == "world":
            w[:, j, 3:6] += ik_ref.point_position(np.asarray(q, dtype=np.float64), link)
    return w.astype(np.float32) if rounded else w


def joint_torques(family, n):
    tau = np.random.default_rng(FAMILIES[family]["seed"] + 103).uniform(-1.0, 1.0, size=(N_MAX, DOF)) * TORQUE_SCALE
    return tau[:n].astype(np.float32)


# A wrench of unit scale (force +-30, torque +-15) moves qd in one sub-step by 2e-4 (median env) on links 1-3, whose joints carry
# the whole arm, 2e-3 on link 4 and 1e-2 on links 5-10 (measured on the reference): scaled so that every link's is about 0.06,
# 30 x QD_TOL — a wrench dropped or put on the wrong body shows at any link
LINK_WRENCH_SCALE = {1: 300.0, 2: 300.0, 3: 300.0, 4: 30.0, 5: 5.0, 6: 5.0, 7: 5.0, 8: 5.0, 9: 5.0, 10: 5.0}


def same_wrench_both_frames(n, link=7, seed=61, point=None, scale=1.0):
    """One physical wrench on `link` at the poses q: (q, world-frame record [n, 1, 9], link-frame record [n, 1, 9]), float64.
    point: the wrench's point in the link's frame, the same for every env (None: one per env within +-1); scale: of force and torque."""
    import link_kinematics_ref as lk
    rng = np.random.default_rng(seed)
    lo, hi = (v.astype(np.float64) for v in ik_ref.limits_f32())
    q = rng.uniform(0.6 * lo, 0.6 * hi, size=(n, DOF)).astype(np.float32).astype(np.float64)
    F, P, T = scale * rng.uniform(-30, 30, (n, 3)), rng.uniform(-1, 1, (n, 3)), scale * rng.uniform(-15, 15, (n, 3))
    if point is not None:
        P = np.broadcast_to(np.asarray(point, dtype=np.float64), (n, 3))
    R, p, _, _ = lk.link_frames(q)
    Rl, pl = R[:, link], p[:, link]
    to_world = lambda v: np.einsum("nij,nj->ni", Rl, v)  # noqa: E731
    world = np.concatenate([to_world(F), pl + to_world(P), to_world(T)], axis=1)[:, None, :]
    local = np.concatenate([F, P, T], axis=1)[:, None, :]
    return q, world, local
