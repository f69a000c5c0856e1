"""Independent float64 reference of pnr_get_joint_states: per joint q̈ and the motor torque of the world step's first sub-step, and
the joints' reaction wrenches.

  * q̈: world_step_ref.accelerations (the float64 oracle's forward dynamics with the motors' table law, the joint losses, the
    caller's joint torques, the contacts' wrenches and the caller's) for PD and inertia-scaled motors; constraint_motor_ref.constrain
    for constraint motors: (qd_plus - qd) / h, qd_plus before the joint limits act.
  * the motor torque: the oracle's table law as world_step_ref.table_law gives it; a constraint joint's is constrain's tau.
    The inertia-scaled law's torque is formed inside the oracle's ABA and not handed out: there the stated identity is used,
    tau_motor = (the reaction's moment along the joint axis) - joint_torque + damping + friction, evaluated in float64.
  * the reaction: a world-frame Newton-Euler sweep over the 11 URDF links (link_kinematics_ref.link_frames with q̈: per link
    F = s acc, N = s alpha, mass s and inertia s 1 about the link's origin) at that q̈, with the oracle's per-body contact wrenches and
    external_force_ref.body_wrenches subtracted: everything distal to joint b summed, shifted to body b's origin and rotated into
    body b's frame.  A different statement of the mechanics from the kernel's body-frame recursion on six merged bodies.

newton_euler_reaction takes a dtype, as inverse_dynamics_ref.newton_euler does: in float32 it is the restatement the bars' float32
floor is measured with (tests/joint_state_cases.py); forward32 restates q̈ the same way, from the Newton-Euler mass matrix and bias.
It reads nothing of pioneer_amd.
"""
import numpy as np

import constraint_motor_ref as cref
import external_force_ref as xref
import ik_ref
import inverse_dynamics_ref as idref
import link_kinematics_ref as lk
import world_step_ref as wref

DOF = 6
LINKS = 11


def contact_wrenches(orc):
    """[n, 6, 6] per body n_b | f_b (body coordinates) of the oracle's contacts at its current states, and who is in contact [n]"""
    f = np.zeros((orc.n, DOF, 6))
    hit = np.zeros(orc.n, dtype=bool)
    if wref.has_contacts(orc):
        for e in range(orc.n):
            hit[e], f[e] = orc.contact_wrenches(e)
    return f, hit


def external_wrenches(orc, specs=(), wrenches=None):
    """[n, 6, 6]: the caller's records at the oracle's current pose (which is the call's q0)"""
    if not len(specs):
        return np.zeros((orc.n, DOF, 6))
    q = orc.dstate["q"].copy()
    return xref.body_wrenches(xref.prepare(specs, wrenches, q), q)


# ---- the Newton-Euler part, in the caller's dtype ------------------------------------------------------------------------------------
def newton_euler_reaction(q, qd, qdd, scales, gravity, fext=None, dtype=np.float64, frame="child", chain=None):
    """[n, 6, 6] in `dtype`: per joint b (Fx, Fy, Fz, Mx, My, Mz), the wrench the parent exerts on body b at body b's origin in body
    b's coordinates (frame="parent": in the parent body's, the mistake the tests tell apart).  fext [n, 6, 6]: per body n_b | f_b in
    body coordinates about the body's origin (contacts plus the caller's), subtracted."""
    T = np.dtype(dtype).type
    chain = chain or lk.load_chain()
    q, qd, qdd, scales = (np.atleast_2d(np.asarray(x, dtype=T)) for x in (q, qd, qdd, scales))
    n = q.shape[0]
    R, p, _, _, al, acc, _, origins = lk.link_frames(q, qd, chain, qdd=qdd, gravity=gravity, dtype=T)
    upstream = idref.joints_upstream(chain)
    R = R[:, ik_ref.revolute_links(chain)[0]]                                 # the six bodies' world rotations
    fe = None if fext is None else np.asarray(fext, dtype=T)
    out = np.zeros((n, DOF, 6), dtype=T)
    for b in range(DOF):
        o = origins[:, b]
        F, N = np.zeros((n, 3), dtype=T), np.zeros((n, 3), dtype=T)
        for l, nj in enumerate(upstream):
            if nj > b:                                                # the link hangs on joint b
                s = scales[:, l:l + 1]
                f = s * acc[:, l]
                F = F + f
                N = N + np.cross(p[:, l] - o, f) + s * al[:, l]
        if fe is not None:
            for c in range(b, DOF):
                fw = np.einsum("nij,nj->ni", R[:, c], fe[:, c, 3:6])
                nw = np.einsum("nij,nj->ni", R[:, c], fe[:, c, 0:3])
                F = F - fw
                N = N - nw - np.cross(origins[:, c] - o, fw)
        Rb = R[:, b] if frame == "child" else (R[:, b - 1] if b > 0 else np.broadcast_to(np.eye(3, dtype=T), (n, 3, 3)))
        out[:, b, 0:3] = np.einsum("nji,nj->ni", Rb, F)
        out[:, b, 3:6] = np.einsum("nji,nj->ni", Rb, N)
    assert out.dtype == np.dtype(dtype)
    return out


def axis_moment(reaction, chain=None):
    """[n, 6]: each joint's reaction moment along its axis (the axis in the child's frame is the URDF's)"""
    chain = chain or lk.load_chain()
    axes = np.array([j["axis"] for j in chain if j["type"] == "revolute"], dtype=reaction.dtype)
    return (reaction[:, :, 3:6] * axes[None]).sum(axis=2)


def forward32(q, qd, scales, gravity, fext, tau, dtype=np.float32):
    """q̈ [n, 6] in `dtype` from the Newton-Euler restatement alone: M q̈ = tau - (bias - Q_ext), with M the Newton-Euler mass
    matrix and bias - Q_ext the axis moments of the reaction at q̈ = 0.  tau: every joint torque the ABA receives."""
    T = np.dtype(dtype).type
    q, qd, scales, tau = (np.asarray(x, dtype=T) for x in (q, qd, scales, tau))
    M = idref.newton_euler_mass_matrix(q, scales, T)
    b = axis_moment(newton_euler_reaction(q, qd, np.zeros_like(q), scales, gravity, fext, T))
    return np.linalg.solve(M, (tau - b)[:, :, None])[:, :, 0].astype(T)


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def joint_states(orc, motors, specs=(), wrenches=None, tau_ext=None, h=1.0 / 240, contacts=True, use_wrenches=True, gravity=None,
                 use_torques=True, frame="child"):
    """The reference at the oracle's current states (left as they are).  Returns a dict: qdd, tau_motor [n, 6], reaction [n, 6, 6],
    total [n, 6] (every joint torque the forward dynamics receives: motor + caller's - losses), fext [n, 6, 6], hit [n], and for
    constraint motors Minv [n, 6, 6] and S.  The keyword switches leave a piece out of the REACTION (not of q̈): what the tests use
    to show that the bars tell such a mistake apart."""
    n = orc.n
    q, qd = orc.dstate["q"].copy(), orc.dstate["qd"].copy()
    tx = np.zeros((n, DOF)) if tau_ext is None else np.asarray(tau_ext, dtype=np.float64)
    fc, hit = contact_wrenches(orc)
    fx = external_wrenches(orc, specs, wrenches)
    law = wref.table_law(orc, motors)
    out = dict(hit=hit, fext=fc + fx)
    S = cref.constraint_set(motors)
    if S:
        assert tau_ext is None and not len(specs)
        sub = cref.constrain(orc, motors, *wref.free_dynamics(orc, motors), h)
        qdd = (sub["qd_plus"] - qd) / h
        law[:, S] = sub["tau"]
        out.update(Minv=sub["Minv"], S=S)
    else:
        qdd = wref.accelerations(orc, motors, fx, None if tau_ext is None else tx)      # (it adds the contacts itself)
    g = orc.d.gravity if gravity is None else gravity
    f_used = (fc if contacts else 0 * fc) + (fx if use_wrenches else 0 * fx)
    reaction = newton_euler_reaction(q, qd, qdd, orc.dstate["mass_scale"], g, f_used, np.float64, frame)
    recovered = axis_moment(reaction) - (tx if use_torques else 0 * tx) + wref.losses(orc)
    tau_motor = np.where(np.isnan(law), recovered, law)
    out.update(qdd=qdd, tau_motor=tau_motor, reaction=reaction, total=tau_motor + tx - wref.losses(orc))
    return out
