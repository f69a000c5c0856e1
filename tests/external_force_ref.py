"""Independent float64 reference of pnr_world_step_wrenches (external forces and torques on links of the arm).

The law is the one stated in include/pioneer_amd.h.  One call is frame_skip sub-steps of length h.  A record is (link, frame)
plus, per env, force[3] | position[3] | torque[3].  The link maps to its dynamic body b (the revolute joints up to the link,
fixed joints merged) and to the link origin's fixed offset d in body coordinates.
    frame "link":   f_b = force,  n_b = (d + position) x force + torque,  constant over the call
    frame "world":  p_b = R_b(q0)^T (position - o_b(q0)) at the call's first pose, then in every sub-step
                    f_b = R_b(q_k)^T force,  n_b = p_b x f_b + R_b(q_k)^T torque
    fext[b] += (n_b, f_b) in the first `hold` sub-steps, on top of the contact wrenches; link 0 (the welded base) does nothing.

Built on the float64 oracle's forward dynamics alone (DynOracle.aba_ext / aba_motor with their fext slot, orc_dyn_motor_torque,
contact_wrenches), which tests/test_dyn_oracle.py validates, in the manner of tests/constraint_motor_ref.py, whose motor
dictionaries and table law it uses; the poses R_b, o_b and the link offsets come from tests/link_kinematics_ref.py (the URDF chain
of tests/golden/urdf_chain.json), not from the oracle or the engine.  The integrator is restated: semi-implicit Euler with the
inelastic joint limits (orc_dyn_substep's).  It reads nothing of pioneer_amd.  Numbers are used as the engine stores them,
rounded to float32.
"""
import ctypes as C

import numpy as np

import constraint_motor_ref as cref
import ik_ref
import link_kinematics_ref as lk
from oracle.binding import OrcDynParams

DOF = 6
NUM_LINKS = 11
FRICTION_EPS = cref.FRICTION_EPS


def body_links():
    """The link whose frame is dynamic body b's frame: the child link of revolute joint b."""
    idx, _, _, _ = ik_ref.revolute_links()
    return list(idx)


def body_of(link):
    """The dynamic body (0..5) a URDF link is part of; -1 for a link welded to the world (link 0, robot:base)."""
    return sum(1 for k in body_links() if k <= link) - 1


def link_offset(link):
    """d: the link origin in its body's coordinates (a constant of the chain: fixed joints only in between)."""
    b = body_of(link)
    R, p, _, _ = lk.link_frames(np.zeros((1, DOF)))
    k = body_links()[b]
    return R[0, k].T @ (p[0, link] - p[0, k])


def body_frames(q):
    """R [n, 6, 3, 3] and o [n, 6, 3]: the six bodies' world rotations and origins at q [n, 6]."""
    R, p, _, _ = lk.link_frames(q)
    k = body_links()
    return R[:, k], p[:, k]


def prepare(specs, wrenches, q0):
    """The records' call-constant parts.  specs: [(link, "link" | "world")]; wrenches [n, K, 9] (force | position | torque);
    q0 [n, 6].  Returns a list of (body, frame, A, B, C) with arrays [n, 3]: frame "link": A = f_b, B = n_b (C unused);
    frame "world": A = force, B = p_b, C = torque.  Records on the welded base are dropped."""
    w = np.asarray(wrenches, dtype=np.float64)
    R0, o0 = body_frames(q0)
    out = []
    for j, (link, frame) in enumerate(specs):
        assert 0 <= link < NUM_LINKS and frame in ("link", "world")
        b = body_of(link)
        if b < 0:
            continue
        F, P, T = w[:, j, 0:3], w[:, j, 3:6], w[:, j, 6:9]
        if frame == "link":
            out.append((b, frame, F, np.cross(link_offset(link) + P, F) + T, None))
        else:
            out.append((b, frame, F, np.einsum("nji,nj->ni", R0[:, b], P - o0[:, b]), T))
    return out


def body_wrenches(records, q):
    """fext [n, 6, 6] (per body: n_b | f_b, body coordinates) of the prepared records at the pose q."""
    n = q.shape[0]
    fext = np.zeros((n, DOF, 6))
    R = None
    for b, frame, A, B, C in records:
        if frame == "link":
            fb, nb = A, B
        else:
            if R is None:
                R, _ = body_frames(q)
            fb = np.einsum("nji,nj->ni", R[:, b], A)
            nb = np.cross(B, fb) + np.einsum("nji,nj->ni", R[:, b], C)
        fext[:, b, 0:3] += nb
        fext[:, b, 3:6] += fb
    return fext


def accelerations(orc, motors, fext, tau_ext=None):
    """qdd [n, 6] at the oracle's current states: the joints' motors (constraint_motor_ref's dictionaries; PD kinds or None), the
    joint losses, the caller's joint torques, the contacts' wrenches plus fext [n, 6, 6]."""
    assert not cref.constraint_set(motors)
    n, d = orc.n, orc.d
    orc.lib.orc_dyn_motor_torque.restype = C.c_double
    scaled = bool(d.pd_inertia_scaled)
    contacts = d.ground_z == d.ground_z or d.obstacle_half_extents[0] > 0 or d.n_scene > 0
    u = OrcDynParams()
    qdd = np.empty((n, DOF))
    for e in range(n):
        q, qd = orc.dstate["q"][e], orc.dstate["qd"][e]
        r_cmd, v_cmd = orc.state["r"][e], orc.state["v"][e].astype(np.float64)
        law = np.array([cref._pd_torque(orc, motors[i], u, r_cmd[i], v_cmd[i], q[i], qd[i], scaled) for i in range(DOF)])
        tau = -orc.dstate["damping"][e] * qd - orc.dstate["friction"][e] * qd / np.sqrt(qd * qd + FRICTION_EPS ** 2)
        if tau_ext is not None:
            tau = tau + tau_ext[e]
        f = fext[e]
        if contacts:
            hit, fc = orc.contact_wrenches(e)
            if hit:
                f = f + fc
        if scaled:
            caps = {cref._f32(m.get("max_force", d.torque_limit)) for m in motors if m is not None and m["kind"] == "pd"}
            assert caps <= {float(d.torque_limit)}, "orc_dyn_aba_motor takes one cap for all joints"
            qdd[e] = orc.aba_motor(tau, law, d.torque_limit, d.gravity, f, e)
        else:
            qdd[e] = orc.aba_ext(tau + law, d.gravity, f, e)
    return qdd


def integrate(orc, qdd, h):
    """semi-implicit Euler with the inelastic joint limits, in place on orc.dstate"""
    q, qd = orc.dstate["q"], orc.dstate["qd"]
    lo, hi = np.array(orc.p.r_lo[:], dtype=np.float64), np.array(orc.p.r_hi[:], dtype=np.float64)
    qdn = qd + h * qdd
    qn = q + h * qdn
    qdn[(qn > hi) & (qdn > 0)] = 0.0
    qdn[(qn < lo) & (qdn < 0)] = 0.0
    orc.dstate["q"], orc.dstate["qd"] = np.clip(qn, lo, hi), qdn


def world_step(orc, motors, specs=(), wrenches=None, tau_ext=None, hold_substeps=0, frame_skip=None, h=1.0 / 240):
    """One World.step of every env of the oracle's batch, in place on orc.dstate.  Returns the sub-steps' qdd."""
    nsub = orc.d.frame_skip if frame_skip is None else frame_skip
    hold = nsub if hold_substeps <= 0 or hold_substeps >= nsub else hold_substeps
    records = prepare(specs, wrenches, orc.dstate["q"].copy()) if len(specs) else []
    tau = None if tau_ext is None else np.asarray(tau_ext, dtype=np.float64)
    zero = np.zeros((orc.n, DOF, 6))
    out = []
    for k in range(nsub):
        fext = body_wrenches(records, orc.dstate["q"]) if k < hold and records else zero
        qdd = accelerations(orc, motors, fext, tau)
        integrate(orc, qdd, h)
        out.append(qdd)
    return out
