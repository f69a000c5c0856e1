"""The float64 reference of one pnr_world_step call, written once, as dyn_world_kernel is: every form of the call (plain, joint
torques, link wrenches, per-env motor targets, the moving sphere, constraint motors) is the one `world_step` below with keyword
arguments, and every GPU test of a world step is held against it.

One sub-step of length h evaluates each joint's motor law, forms the joint losses, adds the caller's torques, collects the contact
and external wrenches, runs the oracle's forward dynamics and integrates with the inelastic joint limits.  The parts a feature
brings are that feature's module: the boxed solve of the constraint motors (tests/constraint_motor_ref.py), the wrench records
(tests/external_force_ref.py), the sphere's forces and integration (tests/moving_sphere_ref.py).

Built on the float64 oracle's forward dynamics alone (DynOracle.aba_ext / aba_motor with their fext slot, orc_dyn_motor_torque,
contact_wrenches), which tests/test_dyn_oracle.py validates; it reads nothing of pioneer_amd.  The integrator is restated:
semi-implicit Euler with the inelastic joint limits (orc_dyn_substep's).

A motor is None (the env-wide law of the oracle's params on the env's command state) or a dict:
    dict(kind="velocity_constraint", target_velocity, max_force)
    dict(kind="position_constraint", target_position, target_velocity, position_gain, velocity_gain, max_force, max_velocity)
    dict(kind="pd", control_mode, target_position, target_velocity, position_gain, velocity_gain, max_force, max_velocity)
with the arguments a constraint motor leaves out at Bullet's values (PNR_BULLET_*).  Numbers are used as the engine stores them,
rounded to float32.
"""
import contextlib
import ctypes as C

import numpy as np

import constraint_motor_ref as cref
import external_force_ref as xref
import moving_sphere_ref as sref
from oracle.binding import OrcDynParams

DOF = 6
FRICTION_EPS = 0.05


def has_contacts(orc):
    d = orc.d
    return bool(d.ground_z == d.ground_z or d.obstacle_half_extents[0] > 0 or d.n_scene > 0)


def losses(orc):
    """[n, 6]: damping qd + friction qd / sqrt(qd^2 + eps^2), the torque the joints lose"""
    qd = orc.dstate["qd"]
    return orc.dstate["damping"] * qd + orc.dstate["friction"] * qd / np.sqrt(qd * qd + FRICTION_EPS ** 2)


def joint_law(orc, m, u, r_cmd, v_cmd, q, qd, uncapped=False):
    """The table law of one joint from the oracle: orc_dyn_motor_torque with the joint's own gains (u: a scratch copy of the params)."""
    C.memmove(C.byref(u), C.byref(orc.d), C.sizeof(OrcDynParams))
    if m is None:
        if orc.d.teleport:
            return 0.0
        r_ref, v_ref = r_cmd, v_cmd
    elif m["kind"] == "pd":
        u.control_mode = int(m["control_mode"])
        u.kp = cref.f32(m.get("position_gain", orc.d.kp)); u.kd = cref.f32(m.get("velocity_gain", orc.d.kd))
        u.torque_limit = cref.f32(m.get("max_force", orc.d.torque_limit))
        u.max_velocity = 0.0 if u.control_mode == 1 else cref.f32(m.get("max_velocity", orc.d.max_velocity))
        r_ref, v_ref = cref.f32(m.get("target_position", 0.0)), cref.f32(m.get("target_velocity", 0.0))
    else:
        return 0.0                                                    # a constraint joint, or a constraint motor with force 0
    if uncapped:
        u.torque_limit = 0.0
    return orc.lib.orc_dyn_motor_torque(C.byref(u), C.c_double(r_ref), C.c_double(v_ref), C.c_double(q), C.c_double(qd))


def _env_law(orc, motors, u, e, uncapped):
    """[6]: joint_law of env e's six joints at its current state and command state"""
    orc.lib.orc_dyn_motor_torque.restype = C.c_double
    q, qd, r, v = orc.dstate["q"][e], orc.dstate["qd"][e], orc.state["r"][e], orc.state["v"][e].astype(np.float64)
    return np.array([joint_law(orc, motors[i], u, r[i], v[i], q[i], qd[i], uncapped) for i in range(DOF)])


def table_law(orc, motors):
    """[n, 6]: the PD table law's torque after its cap (0 for a constraint joint; NaN where the inertia-scaled law applies)"""
    u = OrcDynParams()
    out = np.stack([_env_law(orc, motors, u, e, False) for e in range(orc.n)])
    if orc.d.pd_inertia_scaled:
        out[:, [i for i, m in enumerate(motors) if m is None or m["kind"] == "pd"]] = np.nan
    return out


def _forward(orc, motors, fext, tau_ext):
    """The single per-env loop.  Yields, per env, (aba, tau): the oracle's forward dynamics at the env's current state as a
    function of the joint torques (the contacts' wrenches plus fext [n, 6, 6] inside; under pd_inertia_scaled the motors' uncapped
    law as the acceleration request), and tau = -losses + tau_ext (+ the motors' table law, where it is a torque)."""
    d = orc.d
    scaled = bool(d.pd_inertia_scaled)
    if scaled:
        caps = {cref.f32(m.get("max_force", d.torque_limit)) for m in motors if m is not None and m["kind"] == "pd"}
        assert caps <= {float(d.torque_limit)}, "orc_dyn_aba_motor takes one cap for all joints"
    contacts = has_contacts(orc)
    u = OrcDynParams()
    lost = losses(orc)
    for e in range(orc.n):
        law = _env_law(orc, motors, u, e, scaled)
        tau = -lost[e] if tau_ext is None else -lost[e] + tau_ext[e]
        f = None if fext is None else fext[e]
        if contacts:
            hit, fc = orc.contact_wrenches(e)
            if hit:
                f = fc if f is None else f + fc
        if scaled:
            yield (lambda t, law=law, f=f, e=e: orc.aba_motor(t, law, d.torque_limit, d.gravity, f, e)), tau
        else:
            yield (lambda t, f=f, e=e: orc.aba_ext(t, d.gravity, f, e)), tau + law


def accelerations(orc, motors, fext=None, tau_ext=None):
    """qdd [n, 6] at the oracle's current states: the joints' motors, the joint losses, the caller's joint torques tau_ext [n, 6],
    the contacts' wrenches plus fext [n, 6, 6].  A constraint joint's motor torque is 0."""
    return np.stack([aba(tau) for aba, tau in _forward(orc, motors, fext, tau_ext)])


def free_dynamics(orc, motors):
    """qdd_free [n, 6] = accelerations(orc, motors) and M^-1 [n, 6, 6], column by column from the ABA's affinity in tau,
    ABA(tau + e_j) - ABA(tau)."""
    qdd, Minv = np.empty((orc.n, DOF)), np.empty((orc.n, DOF, DOF))
    eye = np.eye(DOF)
    for e, (aba, tau) in enumerate(_forward(orc, motors, None, None)):
        qdd[e] = aba(tau)
        for j in range(DOF):
            Minv[e, :, j] = aba(tau + eye[j]) - qdd[e]
    return qdd, Minv


def integrate(orc, qd_plus, h):
    """semi-implicit Euler from the new velocities qd_plus [n, 6] with the inelastic joint limits, in place on orc.dstate"""
    lo, hi = np.array(orc.p.r_lo[:], dtype=np.float64), np.array(orc.p.r_hi[:], dtype=np.float64)
    qn = orc.dstate["q"] + h * qd_plus
    qdn = qd_plus.copy()
    qdn[(qn > hi) & (qdn > 0)] = 0.0
    qdn[(qn < lo) & (qdn < 0)] = 0.0
    orc.dstate["q"], orc.dstate["qd"] = np.clip(qn, lo, hi), qdn


@contextlib.contextmanager
def command_targets(orc, targets, joints):
    """targets [n, 12] (position[6] | velocity[6]) stand in for the envs' command state r, v of the joints `joints` (joints on
    the env-wide law) inside the block; the command state is put back afterwards."""
    keep = orc.state["r"].copy(), orc.state["v"].copy()
    for j in joints:
        orc.state["r"][:, j], orc.state["v"][:, j] = targets[:, j], targets[:, DOF + j]
    try:
        yield
    finally:
        orc.state["r"], orc.state["v"] = keep


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def world_step(orc, motors, *, tau_ext=None, wrenches=None, hold_substeps=0, sphere=None, sphere_params=None, targets=None,
               joints=(), storage32=False, frame_skip=None, h=1.0 / 240):
    """One World.step of every env of the oracle's batch, in place on orc.dstate (and on `sphere`): frame_skip sub-steps (default:
    the oracle's) of length h.
        tau_ext [n, 6]           the caller's joint torques
        wrenches (specs, w)      external_force_ref's records, acting in the first hold_substeps sub-steps (<= 0: in all)
        sphere                   moving_sphere_ref's state dict (sphere_params: its contact parameters)
        targets [n, 12], joints  the per-env targets of command_targets, which the joints `joints` track
        storage32                the joints' and the sphere's state rounded to float32 after every sub-step
    Returns one dict per sub-step: a constraint sub-step's record (constraint_motor_ref.constrain) or dict(qdd [n, 6]), and with a
    sphere arm_force [n, 3] (the arm's on the sphere), on_arm, on_static [n] (what the sphere touches).
    Refused, as the kernel refuses them: constraint motors next to torques, wrenches or a sphere; wrenches next to a sphere; a
    motor of its own on a joint that takes per-env targets."""
    nsub = orc.d.frame_skip if frame_skip is None else frame_skip
    hold = nsub if hold_substeps <= 0 or hold_substeps >= nsub else hold_substeps
    specs, w = ((), None) if wrenches is None else wrenches
    S = cref.constraint_set(motors)
    assert not (S and (tau_ext is not None or wrenches is not None or sphere is not None))
    assert sphere is None or wrenches is None
    assert targets is None or all(motors[j] is None for j in joints)
    records = xref.prepare(specs, w, orc.dstate["q"].copy()) if len(specs) else []
    tau = None if tau_ext is None else np.asarray(tau_ext, dtype=np.float64)
    p = None if sphere is None else sref.params_of(orc, sphere_params)
    out = []
    with command_targets(orc, targets, joints if targets is not None else ()):
        for k in range(nsub):
            rec = {}
            fext = xref.body_wrenches(records, orc.dstate["q"]) if k < hold and records else None
            if sphere is not None:
                Fs, on_static = sref.static_force(orc, sphere, p)
                Fa, fext, on_arm = sref.arm_forces(orc, sphere, p)
                rec.update(arm_force=Fa, on_arm=on_arm, on_static=on_static)
            if S:
                rec.update(cref.constrain(orc, motors, *free_dynamics(orc, motors), h))
                qd_plus = rec["qd_plus"]
            else:
                rec["qdd"] = accelerations(orc, motors, fext, tau)
                qd_plus = orc.dstate["qd"] + h * rec["qdd"]
            integrate(orc, qd_plus, h)
            if sphere is not None:
                sref.integrate(sphere, Fs + Fa, p, float(orc.d.gravity), h)
            if storage32:
                orc.dstate["q"], orc.dstate["qd"] = _f32(orc.dstate["q"]), _f32(orc.dstate["qd"])
                if sphere is not None:
                    sphere["x"], sphere["v"] = _f32(sphere["x"]), _f32(sphere["v"])
            out.append(rec)
    return out
