"""Independent float64 reference of the constraint joint motor in pnr_world_step (PNR_CONTROL_*_CONSTRAINT).

The law is the one stated in include/pioneer_amd.h.  Per sub-step of length h, with S the constraint joints whose force is > 0
(force 0 is no motor), qdd_free the forward dynamics with tau_S = 0 and M the joint-space mass matrix:
    qd+ = qd + h (qdd_free + M^-1 tau),   tau = 0 off S,
    per i in S:  qd+_i = rhs_i with |tau_i| <= F_i,  or  tau_i = +F_i with qd+_i <= rhs_i,  or  tau_i = -F_i with qd+_i >= rhs_i,
    rhs_i = v*  (VELOCITY)     rhs_i = clip(kp (q* - q) / h + qd + kd (v* - qd), +-maxVelocity)  (POSITION; maxVelocity > 0).

This module is the constraint half of a sub-step (`constrain`); the rest of the sub-step (the other joints' motors, losses,
contacts, the integrator) is tests/world_step_ref.py's, whose world_step calls it.  It reads nothing of pioneer_amd and restates
neither a mass-matrix algorithm nor a solver:
  * qdd_free and M^-1 are world_step_ref.free_dynamics' (the float64 oracle's ABA and its affinity in tau);
  * the boxed problem is solved by EXHAUSTIVE ENUMERATION of the 3^|S| patterns (each joint of S free, at +F or at -F): for every
    pattern the free joints' torques follow from one linear solve, and the pattern is consistent when those torques are within
    their forces and the clamped joints stay short of rhs on their own side.  For an SPD mass matrix exactly one pattern is.
The enumeration is batched over envs: the 2^|S| free sets each take one numpy.linalg.solve with the sign choices of the clamped
joints as right-hand sides.

The motors are tests/world_step_ref.py's dictionaries; the arguments a constraint motor leaves out are at Bullet's values
(PNR_BULLET_*).  Numbers are used as the engine stores them, rounded to float32.
"""
import itertools

import numpy as np

DOF = 6
BULLET = dict(target_velocity=0.0, position_gain=0.1, velocity_gain=1.0, max_force=1e5, max_velocity=0.0)


def f32(x):
    return float(np.float32(x))


def constraint_set(motors):
    """S: the joints on a constraint motor with force > 0."""
    return [i for i, m in enumerate(motors) if m is not None and m["kind"].endswith("_constraint")
            and f32(m.get("max_force", BULLET["max_force"])) > 0]


def targets(orc, motors, h):
    """rhs [n, 6] of the stated law (NaN off the constraint joints) and whether maxVelocity capped it [n, 6]."""
    q, qd = orc.dstate["q"], orc.dstate["qd"]
    rhs = np.full((orc.n, DOF), np.nan)
    capped = np.zeros((orc.n, DOF), dtype=bool)
    for i in constraint_set(motors):
        m = dict(BULLET, **motors[i])
        if m["kind"] == "velocity_constraint":
            rhs[:, i] = f32(m["target_velocity"])
            continue
        kp, kd, vmax = f32(m["position_gain"]), f32(m["velocity_gain"]), f32(m["max_velocity"])
        v = kp * (f32(m["target_position"]) - q[:, i]) / h + qd[:, i] + kd * (f32(m["target_velocity"]) - qd[:, i])
        if vmax > 0:
            capped[:, i] = np.abs(v) > vmax
            v = np.clip(v, -vmax, vmax)
        rhs[:, i] = v
    return rhs, capped


def solve_boxed(A, b, rhs, F):
    """The boxed problem  v = b + A tau,  per joint v = rhs with |tau| <= F, or tau = +-F with v short of rhs on that side,
    for A [n, m, m] SPD, b, rhs [n, m], F [m], by enumeration of all 3^m patterns.

    Returns tau [n, m], v [n, m], pattern [n, m] (0 free, +1 at +F, -1 at -F), margin [n], consistent [n]: the number of
    patterns that satisfy the conditions (margin >= 0), and slack [n, m].  slack is each joint's complementarity slack in the
    chosen pattern in velocity units: rhs - v (or v - rhs) of a clamped joint, A_ii (F_i - |tau_i|) of a free one — the velocity
    its remaining torque could still add; margin is the smallest of them."""
    n, m = b.shape
    best = np.full(n, -np.inf)
    consistent = np.zeros(n, dtype=np.int64)
    tau_out, pat_out, slack_out = np.zeros((n, m)), np.zeros((n, m), dtype=np.int64), np.zeros((n, m))
    diag = A[:, np.arange(m), np.arange(m)]
    for free in itertools.product((True, False), repeat=m):
        f = [i for i in range(m) if free[i]]
        c = [i for i in range(m) if not free[i]]
        k = 2 ** len(c)
        signs = np.array(list(itertools.product((1.0, -1.0), repeat=len(c)))).reshape(k, len(c))
        tau = np.zeros((n, k, m))
        tau[:, :, c] = signs * F[c]
        if f:
            R = (rhs[:, f] - b[:, f])[:, :, None] - A[:, f][:, :, c] @ tau[:, :, c].transpose(0, 2, 1)  # [n, |f|, k]
            tau[:, :, f] = np.linalg.solve(A[:, f][:, :, f], R).transpose(0, 2, 1)
        v = b[:, None, :] + np.einsum("nij,nkj->nki", A, tau)
        slack = np.empty((n, k, m))
        slack[:, :, f] = diag[:, None, f] * (F[f] - np.abs(tau[:, :, f]))
        slack[:, :, c] = signs * (rhs[:, None, c] - v[:, :, c])
        margin = slack.min(axis=2) if m else np.zeros((n, k))                                            # [n, k]
        consistent += (margin >= 0).sum(axis=1)
        j = margin.argmax(axis=1)
        mj = margin[np.arange(n), j]
        better = mj > best
        best = np.where(better, mj, best)
        tau_out[better] = tau[np.arange(n), j][better]
        pat = np.zeros((k, m), dtype=np.int64)
        pat[:, c] = signs
        pat_out[better] = pat[j][better]
        slack_out[better] = slack[np.arange(n), j][better]
    return tau_out, b + np.einsum("nij,nj->ni", A, tau_out), pat_out, best, consistent, slack_out


def constrain(orc, motors, qdd_free, Minv, h=1.0 / 240):
    """The constraint half of a sub-step at the oracle's current states, from the forward dynamics with tau_S = 0 and M^-1
    (world_step_ref.free_dynamics); nothing is integrated.  Returns a dict: S, tau [n, |S|], qd_plus [n, 6] (before the joint limits
    act), rhs, capped [n, 6], pattern, slack [n, |S|], margin, consistent [n], Minv [n, 6, 6], qdd_free, b [n, 6], F [|S|]."""
    S = constraint_set(motors)
    rhs, capped = targets(orc, motors, h)
    b = orc.dstate["qd"] + h * qdd_free
    F = np.array([f32(dict(BULLET, **motors[i])["max_force"]) for i in S])
    tau, _, pattern, margin, consistent, slack = solve_boxed(h * Minv[:, S][:, :, S], b[:, S], rhs[:, S], F)
    qd_plus = b + h * np.einsum("nij,nj->ni", Minv[:, :, S], tau)
    return dict(S=S, tau=tau, qd_plus=qd_plus, rhs=rhs, capped=capped, pattern=pattern, margin=margin, consistent=consistent, slack=slack,
                Minv=Minv, qdd_free=qdd_free, b=b, F=F)
