"""Independent float64 reference of the grip (pnr_set_body_grip_params / pnr_set_body_grip): each env's moving sphere held at a
point of link robot:pointer by a soft point-to-point constraint with a force cap.  The law is the one stated in
include/pioneer_amd.h.  Per sub-step of length h, at the state the sub-step starts from, in every env whose max_force is > 0 and
whose mass is > 0:
    c_a = kTip + anchor + (radius + pointer_radius) direction     (moving body 5's frame)
    p_a = p_5 + R_5 c_a,  v_a = v_5 + w_5 x (R_5 c_a)             (world; as a contact sample's position and velocity)
    F_r = -grip_kp (x - p_a) - grip_kd (v - v_a),   F = F_r min(1, max_force / |F_r|)
    +F on the sphere, -F on body 5 at c_a (fext[5] = (c_a x R_5^T(-F), R_5^T(-F))); the gripped sphere takes no force from the
    arm's samples; the static world's force on it stays.

tests/world_step_ref.py cannot take a new keyword, so `world_step` below restates its sphere branch out of that module's public
pieces (accelerations, integrate, command_targets) and of tests/moving_sphere_ref.py's (static_force, arm_forces, integrate), with
the same `storage32` switch.  With nothing gripped it reproduces world_step_ref.world_step(sphere=...) to the last bit, which
tests/test_grip_cpu.py asserts, so the copy cannot drift unnoticed.  It reads nothing of pioneer_amd.
"""
import numpy as np

import external_force_ref as ext
import link_kinematics_ref as lk
import moving_sphere_ref as sref
import world_step_ref as wref

DOF = 6
K_TIP = np.array([3.6, 0.0, 1.9])                        # the pointer link's origin in moving body 5's frame (the URDF's tip offset)
POINTER_BODY = 5
DEFAULTS = dict(anchor=(0.0, 0.0, 0.0), direction=tuple(K_TIP / np.linalg.norm(K_TIP)), grip_kp=None, grip_kd=None)   # None: the sphere's


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def geometry_of(params=None):
    """anchor and direction as the engine stores them: float32 numbers, a non-zero direction normalised (in float64, then rounded once)"""
    p = dict(DEFAULTS, **(params or {}))
    d = _f32(p["direction"])
    if np.any(d != 0):
        d = d / np.linalg.norm(d)
    return dict(anchor=_f32(p["anchor"]), direction=_f32(d))


def params_of(sphere_params, params=None):
    """The grip's params as the engine resolves and stores them: geometry_of's, and grip_kp / grip_kd as float32 numbers, which default
    to the sphere's resolved contact gains (`sphere_params`: moving_sphere_ref.params_of's dict)."""
    p = dict(DEFAULTS, **(params or {}))
    kp = sphere_params["contact_kp"] if p["grip_kp"] is None else p["grip_kp"]
    kd = sphere_params["contact_kd"] if p["grip_kd"] is None else p["grip_kd"]
    return dict(geometry_of(params), grip_kp=float(_f32(kp)), grip_kd=float(_f32(kd)))


def anchor_local(radius, pointer_radius, gp):
    """c_a [n, 3]: the anchor point in moving body 5's frame, for the envs' radii [n]"""
    reach = np.asarray(radius, dtype=np.float64) + float(pointer_radius)
    return K_TIP[None] + gp["anchor"][None] + reach[:, None] * gp["direction"][None]


def anchor_kinematics(q, qd, radius, pointer_radius, gp):
    """(c_a, p_a, v_a [n, 3], R_5 [n, 3, 3]) at the joints q, qd [n, 6]"""
    R, o, v, w = lk.link_frames(np.asarray(q, dtype=np.float64), np.asarray(qd, dtype=np.float64))
    k = ext.body_links()[POINTER_BODY]
    c = anchor_local(radius, pointer_radius, gp)
    rc = np.einsum("nij,nj->ni", R[:, k], c)
    return c, o[:, k] + rc, v[:, k] + np.cross(w[:, k], rc), R[:, k]


def held(s, max_force):
    return (np.asarray(max_force) > 0) & (s["m"] > 0)


def grip_force(orc, s, max_force, gp):
    """dict(F [n, 3] on the spheres (0 where not held), F_r [n, 3] before the cap (everywhere), fext [n, 6, 6] the reaction on the
    arm's bodies, c_a, p_a, R_5, held [n]) at the oracle's joints"""
    fmax = np.asarray(max_force, dtype=np.float64)
    c, pa, va, R5 = anchor_kinematics(orc.dstate["q"], orc.dstate["qd"], s["r"], orc.d.pointer_radius, gp)
    Fr = -gp["grip_kp"] * (s["x"] - pa) - gp["grip_kd"] * (s["v"] - va)
    length = np.linalg.norm(Fr, axis=1)
    on = held(s, fmax)
    scale = np.where(length > 0, np.minimum(1.0, np.where(on, fmax, 0.0) / np.where(length > 0, length, 1.0)), 1.0)
    F = np.where(on[:, None], scale[:, None] * Fr, 0.0)
    fb = np.einsum("nji,nj->ni", R5, -F)                               # R_5^T (-F)
    fext = np.zeros((len(F), DOF, 6))
    fext[:, POINTER_BODY, 0:3] = np.cross(c, fb)
    fext[:, POINTER_BODY, 3:6] = fb
    return dict(F=F, F_r=Fr, fext=fext, c_a=c, p_a=pa, R_5=R5, held=on)


def world_step(orc, motors, *, sphere, max_force, grip_params=None, sphere_params=None, tau_ext=None, targets=None, joints=(),
               storage32=False, frame_skip=None, h=1.0 / 240):
    """world_step_ref.world_step(sphere=...) with the grip: one World.step of every env of the oracle's batch, in place on
    orc.dstate and `sphere`.  max_force [n]: the envs' grip words (<= 0: released).  Returns dict(force [n, 3]: the grip's force on
    the sphere in the last sub-step, 0 for an env that is not held; records: one dict per sub-step with qdd, arm_force, grip_force,
    grip_raw (F_r), on_arm, on_static, held)."""
    nsub = orc.d.frame_skip if frame_skip is None else frame_skip
    assert not wref.cref.constraint_set(motors)
    assert targets is None or all(motors[j] is None for j in joints)
    tau = None if tau_ext is None else np.asarray(tau_ext, dtype=np.float64)
    p = sref.params_of(orc, sphere_params)
    gp = params_of(p, grip_params)
    fmax = np.asarray(max_force, dtype=np.float64)
    records = []
    force = np.zeros((orc.n, 3))
    with wref.command_targets(orc, targets, joints if targets is not None else ()):
        for _ in range(nsub):
            Fs, on_static = sref.static_force(orc, sphere, p)
            Fa, fext, on_arm = sref.arm_forces(orc, sphere, p)
            g = grip_force(orc, sphere, fmax, gp)
            on = g["held"]
            if on.any():                                               # (nothing held: not one operation more than world_step_ref's)
                Fa[on], fext[on], on_arm = 0.0, 0.0, on_arm & ~on       # a gripped sphere takes no arm contact from any sample
                Fa[on] += g["F"][on]
                fext[on] += g["fext"][on]
            qdd = wref.accelerations(orc, motors, fext, tau)
            wref.integrate(orc, orc.dstate["qd"] + h * qdd, h)
            sref.integrate(sphere, Fs + Fa, p, float(orc.d.gravity), h)
            if storage32:
                orc.dstate["q"], orc.dstate["qd"] = _f32(orc.dstate["q"]), _f32(orc.dstate["qd"])
                sphere["x"], sphere["v"] = _f32(sphere["x"]), _f32(sphere["v"])
            force = g["F"]
            records.append(dict(qdd=qdd, arm_force=Fa - g["F"], grip_force=g["F"], grip_raw=g["F_r"], on_arm=on_arm, on_static=on_static, held=on))
    return dict(force=force, records=records)
