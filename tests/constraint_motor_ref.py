"""Independent float64 reference of the constraint joint motor in pnr_world_step (PNR_CONTROL_*_CONSTRAINT).

The law is the one stated in include/pioneer_amd.h.  Per sub-step of length h, with S the constraint joints whose force is > 0
(force 0 is no motor), qdd_free the forward dynamics with tau_S = 0 and M the joint-space mass matrix:
    qd+ = qd + h (qdd_free + M^-1 tau),   tau = 0 off S,
    per i in S:  qd+_i = rhs_i with |tau_i| <= F_i,  or  tau_i = +F_i with qd+_i <= rhs_i,  or  tau_i = -F_i with qd+_i >= rhs_i,
    rhs_i = v*  (VELOCITY)     rhs_i = clip(kp (q* - q) / h + qd + kd (v* - qd), +-maxVelocity)  (POSITION; maxVelocity > 0).

Built on the float64 oracle's forward dynamics alone (DynOracle.aba_ext / aba_motor, motor_torque, contact_wrenches), which
tests/test_dyn_oracle.py validates; it reads nothing of pioneer_amd and restates neither a mass-matrix algorithm nor a solver:
  * qdd_free is one ABA call; M^-1 comes column by column from the ABA's affinity in tau, ABA(tau + e_j) - ABA(tau);
  * the boxed problem is solved by EXHAUSTIVE ENUMERATION of the 3^|S| patterns (each joint of S free, at +F or at -F): for every
    pattern the free joints' torques follow from one linear solve, and the pattern is consistent when those torques are within
    their forces and the clamped joints stay short of rhs on their own side.  For an SPD mass matrix exactly one pattern is.
The enumeration is batched over envs: the 2^|S| free sets each take one numpy.linalg.solve with the sign choices of the clamped
joints as right-hand sides.

A motor is None (the env-wide law of the oracle's params on the env's command state) or a dict:
    dict(kind="velocity_constraint", target_velocity, max_force)
    dict(kind="position_constraint", target_position, target_velocity, position_gain, velocity_gain, max_force, max_velocity)
    dict(kind="pd", control_mode, target_position, target_velocity, position_gain, velocity_gain, max_force, max_velocity)
with the arguments a constraint motor leaves out at Bullet's values (PNR_BULLET_*).  Numbers are used as the engine stores them,
rounded to float32.
"""
import ctypes as C
import itertools

import numpy as np

from oracle.binding import OrcDynParams

DOF = 6
FRICTION_EPS = 0.05
BULLET = dict(target_velocity=0.0, position_gain=0.1, velocity_gain=1.0, max_force=1e5, max_velocity=0.0)


def _f32(x):
    return float(np.float32(x))


def constraint_set(motors):
    """S: the joints on a constraint motor with force > 0."""
    return [i for i, m in enumerate(motors) if m is not None and m["kind"].endswith("_constraint")
            and _f32(m.get("max_force", BULLET["max_force"])) > 0]


def _pd_torque(orc, m, u, r_cmd, v_cmd, q, qd, uncapped):
    """The table law of joint i from the oracle: orc_dyn_motor_torque with the joint's own gains (u: a scratch copy of the params)."""
    C.memmove(C.byref(u), C.byref(orc.d), C.sizeof(OrcDynParams))
    if m is None:
        if orc.d.teleport:
            return 0.0
        r_ref, v_ref = r_cmd, v_cmd
    elif m["kind"] == "pd":
        u.control_mode = int(m["control_mode"])
        u.kp = _f32(m.get("position_gain", orc.d.kp)); u.kd = _f32(m.get("velocity_gain", orc.d.kd))
        u.torque_limit = _f32(m.get("max_force", orc.d.torque_limit))
        u.max_velocity = 0.0 if u.control_mode == 1 else _f32(m.get("max_velocity", orc.d.max_velocity))
        r_ref, v_ref = _f32(m.get("target_position", 0.0)), _f32(m.get("target_velocity", 0.0))
    else:
        return 0.0                                                    # a constraint joint, or a constraint motor with force 0
    if uncapped:
        u.torque_limit = 0.0
    return orc.lib.orc_dyn_motor_torque(C.byref(u), C.c_double(r_ref), C.c_double(v_ref), C.c_double(q), C.c_double(qd))


def free_dynamics(orc, motors):
    """qdd_free [n, 6] and M^-1 [n, 6, 6] at the oracle's current states, the constraint joints' motor torque at 0."""
    n, d = orc.n, orc.d
    orc.lib.orc_dyn_motor_torque.restype = C.c_double
    scaled = bool(d.pd_inertia_scaled)
    if scaled:
        caps = {_f32(m.get("max_force", d.torque_limit)) for m in motors if m is not None and m["kind"] == "pd"}
        assert caps <= {float(d.torque_limit)}, "orc_dyn_aba_motor takes one cap for all joints"
    contacts = d.ground_z == d.ground_z or d.obstacle_half_extents[0] > 0 or d.n_scene > 0
    u = OrcDynParams()
    qdd, Minv = np.empty((n, DOF)), np.empty((n, DOF, DOF))
    eye = np.eye(DOF)
    for e in range(n):
        q, qd = orc.dstate["q"][e], orc.dstate["qd"][e]
        r_cmd, v_cmd = orc.state["r"][e], orc.state["v"][e].astype(np.float64)
        law = np.array([_pd_torque(orc, motors[i], u, r_cmd[i], v_cmd[i], q[i], qd[i], scaled) for i in range(DOF)])
        tau = -orc.dstate["damping"][e] * qd - orc.dstate["friction"][e] * qd / np.sqrt(qd * qd + FRICTION_EPS ** 2)
        fext = None
        if contacts:
            hit, f = orc.contact_wrenches(e)
            fext = f if hit else None
        if scaled:
            def aba(t):
                return orc.aba_motor(t, law, d.torque_limit, d.gravity, fext, e)
        else:
            tau = tau + law

            def aba(t):
                return orc.aba_ext(t, d.gravity, fext, e)
        qdd[e] = aba(tau)
        for j in range(DOF):
            Minv[e, :, j] = aba(tau + eye[j]) - qdd[e]
    return qdd, Minv


def targets(orc, motors, h):
    """rhs [n, 6] of the stated law (NaN off the constraint joints) and whether maxVelocity capped it [n, 6]."""
    q, qd = orc.dstate["q"], orc.dstate["qd"]
    rhs = np.full((orc.n, DOF), np.nan)
    capped = np.zeros((orc.n, DOF), dtype=bool)
    for i in constraint_set(motors):
        m = dict(BULLET, **motors[i])
        if m["kind"] == "velocity_constraint":
            rhs[:, i] = _f32(m["target_velocity"])
            continue
        kp, kd, vmax = _f32(m["position_gain"]), _f32(m["velocity_gain"]), _f32(m["max_velocity"])
        v = kp * (_f32(m["target_position"]) - q[:, i]) / h + qd[:, i] + kd * (_f32(m["target_velocity"]) - qd[:, i])
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


def substep(orc, motors, h=1.0 / 240):
    """One sub-step of every env of the oracle's batch, in place on orc.dstate.  Returns a dict: S, tau [n, |S|], qd_plus [n, 6]
    (before the joint limits act), rhs, capped [n, 6], pattern, slack [n, |S|], margin, consistent [n], Minv [n, 6, 6], qdd_free [n, 6]."""
    S = constraint_set(motors)
    qdd_free, Minv = free_dynamics(orc, motors)
    rhs, capped = targets(orc, motors, h)
    q, qd = orc.dstate["q"], orc.dstate["qd"]
    b = qd + h * qdd_free
    F = np.array([_f32(dict(BULLET, **motors[i])["max_force"]) for i in S])
    tau, _, pattern, margin, consistent, slack = solve_boxed(h * Minv[:, S][:, :, S], b[:, S], rhs[:, S], F)
    qd_plus = b + h * np.einsum("nij,nj->ni", Minv[:, :, S], tau)
    # semi-implicit Euler with the inelastic joint limits (orc_dyn_substep)
    lo, hi = np.array(orc.p.r_lo[:], dtype=np.float64), np.array(orc.p.r_hi[:], dtype=np.float64)
    qn = q + h * qd_plus
    qdn = qd_plus.copy()
    qdn[(qn > hi) & (qdn > 0)] = 0.0
    qdn[(qn < lo) & (qdn < 0)] = 0.0
    orc.dstate["q"], orc.dstate["qd"] = np.clip(qn, lo, hi), qdn
    return dict(S=S, tau=tau, qd_plus=qd_plus, rhs=rhs, capped=capped, pattern=pattern, margin=margin, consistent=consistent, slack=slack,
                Minv=Minv, qdd_free=qdd_free, b=b, F=F)


def world_step(orc, motors, frame_skip=None, h=1.0 / 240):
    """frame_skip sub-steps (default: the oracle's); returns the sub-steps' dicts."""
    return [substep(orc, motors, h) for _ in range(orc.d.frame_skip if frame_skip is None else frame_skip)]
