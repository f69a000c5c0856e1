"""The input sets of the constraint-motor tests, shared by the CPU tests (which assert on the float64 reference that the inputs
bite) and the GPU tests (which run the kernel on exactly these inputs), and deliberately WRONG solvers of the boxed problem that
the CPU tests use to show what the inputs tell apart.  Nothing here is a reference: that is tests/world_step_ref.py with
tests/constraint_motor_ref.py.
"""
import numpy as np

import oracle_cases as ocases
from oracle import DynOracle

DOF = 6
H = 1.0 / 240


def vel(v, f):
    return dict(kind="velocity_constraint", target_velocity=v, max_force=f)


# gravity, randomised link scales, friction and damping everywhere; no contacts (tests/test_gpu_constraint_motor.py's saturated
# test covers the contact wrenches inside qdd_free)
CASES = {
    # six velocity motors whose forces are of the size the targets need: every joint is free, at +F and at -F in a share of the envs
    "mixed": dict(seed=11, frame_skip=1, frac=0.8, qd=1.5, steps=3, engine=dict(randomize=True),
                  motors=[vel(0.5, 3e4), vel(-0.4, 6e4), vel(0.6, 2e4), vel(-1.0, 300.0), vel(0.8, 800.0), vel(1.2, 300.0)]),
    # S = {0, 2, 3, 5}: two position motors with gains of their own and a maxVelocity that caps rhs, joint 1 on a PD motor with
    # its own gains, joint 4 uncommanded (the env-wide PD law on the command state, which `command_steps` vector steps moved)
    "subset": dict(seed=12, frame_skip=1, frac=0.8, qd=1.5, steps=2, command_steps=3, engine=dict(randomize=True),
                   motors=[dict(kind="position_constraint", target_position=0.3, target_velocity=0.2, position_gain=0.004,
                                velocity_gain=0.5, max_force=2e4, max_velocity=0.75),
                           dict(kind="pd", control_mode=0, target_position=-0.2, target_velocity=0.1, position_gain=9000.0,
                                velocity_gain=700.0, max_force=2.5e4, max_velocity=0.0),
                           vel(0.6, 2e4),
                           dict(kind="position_constraint", target_position=-0.5, position_gain=0.003, velocity_gain=0.8,
                                max_force=300.0, max_velocity=1.0),
                           None,
                           vel(1.2, 300.0)]),
    # one world step of ten sub-steps, free-running: the motors pull the joints onto their targets within the step, so the
    # pattern changes between sub-steps
    "skip10": dict(seed=13, frame_skip=10, frac=0.7, qd=1.5, steps=1, engine=dict(randomize=True),
                   motors=[vel(0.5, 1.2e5), vel(-0.4, 2.4e5), vel(0.6, 8e4), vel(-1.0, 1200.0), vel(0.8, 3200.0), vel(1.2, 1200.0)]),
    # the inertia-scaled env-wide law (an acceleration request scaled inside the ABA) on joints 1, 3, 4 next to constraint motors
    "scaled": dict(seed=14, frame_skip=1, frac=0.8, qd=1.5, steps=2, command_steps=3,
                   engine=dict(randomize=True, pd_inertia_scaled=True, pd_kp=400.0, pd_kd=40.0, torque_limit=2e4),
                   motors=[vel(0.5, 3e4), None, vel(0.6, 2e4), None, None, vel(1.2, 300.0)]),
}
GRAVITY = 9.81


def make_oracle(case, n):
    c = CASES[case]
    return ocases.make_oracle(c["seed"], n, c["frame_skip"], GRAVITY, c["engine"], c.get("command_steps", 0))


def states(case, n, step):
    """(q, qd) [n, 6] float32 of re-randomised step `step`: q uniform within frac x the limits, qd uniform in +-qd."""
    c = CASES[case]
    rng = np.random.default_rng([c["seed"], n, step])
    lo, hi = _limits()
    q = rng.uniform(c["frac"] * lo, c["frac"] * hi, size=(n, DOF)).astype(np.float32)
    qd = rng.uniform(-c["qd"], c["qd"], size=(n, DOF)).astype(np.float32)
    return q, qd


_LIMITS = []


def _limits():
    if not _LIMITS:
        orc = DynOracle(1)
        _LIMITS.append((orc.r_lo.astype(np.float64), orc.r_hi.astype(np.float64)))
    return _LIMITS[0]


# ---- wrong solvers of  v = b + A tau  (A = h M^-1 over S, SPD), each a mistake a kernel could make ----------------------------
def clip_once(A, b, rhs, F):
    """the all-free torques, clipped once: ignores what a clamped joint's lost torque does to the others"""
    tau = np.clip(np.linalg.solve(A, (rhs - b)[:, :, None])[:, :, 0], -F, F)
    return b + np.einsum("nij,nj->ni", A, tau)


def decoupled(A, b, rhs, F):
    """a diagonal mass matrix: every joint solved alone"""
    Mh = np.linalg.inv(A)                                             # M / h over S
    tau = np.clip(Mh[:, np.arange(A.shape[1]), np.arange(A.shape[1])] * (rhs - b), -F, F)
    return b + np.einsum("nij,nj->ni", A, tau)


def active_set(A, b, rhs, F, max_passes):
    """A float64 active-set iteration from the all-free pattern: each pass solves the free joints' torques, clamps those beyond
    their force and frees the clamped ones whose velocity passed rhs; at most max_passes passes, the last one's solve standing.
    Returns v [n, m] and the number of passes each env took."""
    n, m = b.shape
    v_out, passes = np.empty((n, m)), np.empty(n, dtype=np.int64)
    for e in range(n):
        free = np.ones(m, dtype=bool)
        tau = np.zeros(m)
        for p in range(max_passes):
            f, c = np.flatnonzero(free), np.flatnonzero(~free)
            if len(f):
                tau[f] = np.linalg.solve(A[e][np.ix_(f, f)], rhs[e, f] - b[e, f] - A[e][np.ix_(f, c)] @ tau[c])
            v = b[e] + A[e] @ tau
            over = free & (np.abs(tau) > F)
            back = ~free & (np.where(tau > 0, v > rhs[e], v < rhs[e]))
            if not (over.any() or back.any()):
                break
            tau[over] = np.sign(tau[over]) * F[over]
            free = (free & ~over) | back
        v_out[e], passes[e] = v, p + 1
    return v_out, passes
