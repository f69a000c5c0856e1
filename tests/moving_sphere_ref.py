"""Independent float64 reference of the moving sphere (pnr_set_body_params; one sphere per env that the world step integrates with
the arm).  The law is the one stated in include/pioneer_amd.h: a point mass with a radius, no orientation, no spin (rolling is
not modelled).  Per sub-step of length h, every force at the state the sub-step starts from:
    static world   depth = radius - sdf, fn = kp depth - kd (v . n); where depth > 0 and fn > 0:
                   F += fn n - friction fn v_t / sqrt(|v_t|^2 + slip_eps^2), v_t = v - (v . n) n
    arm samples    d = x - p_s, depth = radius + r_s - |d|, n = d / |d| ((0, 0, 1) at |d| = 0), fn = kp depth - kd ((v - v_s) . n);
                   where depth > 0 and fn > 0: +fn n on the sphere, -fn n on the sample's body at the sample's centre
    integration    v += h (F / m - linear_damping v - g z^), x += h v; the joints as tests/world_step_ref.py integrates them
An env with mass <= 0 has no sphere.

This module is the sphere's own law: the forces (`static_force`, `arm_forces`) and `integrate`.  The reference of the call is
tests/world_step_ref.py's world_step(sphere=...), whose forward dynamics take the sphere's reactions in their fext slot and whose
`storage32` rounds the sphere's and the joints' state to float32 after every sub-step: the reference's own float32-storage
deviation is what the GPU test's sphere bars are taken from.  Built on the oracle's sample table (DynOracle.contact_samples) and
on the URDF chain's poses and velocities (tests/link_kinematics_ref.py); the static world's signed distances and normals are
tests/contact_query_ref.py's body_distance.  It reads nothing of pioneer_amd.
"""
import numpy as np

import contact_query_ref as cq
import external_force_ref as ext
import link_kinematics_ref as lk

DOF = 6
DEFAULTS = dict(contact_kp=None, contact_kd=None, friction=0.5, slip_eps=0.05, linear_damping=0.0)      # None: the handle's


def params_of(orc, params=None):
    p = dict(DEFAULTS, **(params or {}))
    if p["contact_kp"] is None:
        p["contact_kp"] = float(orc.d.contact_kp)
    if p["contact_kd"] is None:
        p["contact_kd"] = float(orc.d.contact_kd)
    return p


def sphere(x, v, m, r):
    """the spheres' state as this module carries it: float64 copies of x, v [n, 3], m, r [n]"""
    return dict(x=np.array(x, dtype=np.float64), v=np.array(v, dtype=np.float64), m=np.array(m, dtype=np.float64), r=np.array(r, dtype=np.float64))


def from_words(w):
    """[8, n] planar words (pnr_get_body_state) -> the state dict"""
    w = np.asarray(w, dtype=np.float64)
    return sphere(w[0:3].T, w[3:6].T, w[6], w[7])


# ---- the static world ----------------------------------------------------------------------------------------------------------
def static_bodies(orc):
    """the oracle's static world as contact_query_ref's body records: the ground, the obstacle box, then the scene's bodies"""
    d = orc.d
    out = []
    if d.ground_z == d.ground_z:
        out.append(cq.plane((0.0, 0.0, 1.0), (0.0, 0.0, d.ground_z)))
    if np.all(np.array(d.obstacle_half_extents[:]) > 0):
        out.append(cq.box(d.obstacle_half_extents[:], d.obstacle_position[:]))
    for i in range(d.n_scene):
        b = d.scene[i]
        if b.shape == 1:
            out.append(cq.plane(b.size[:], b.position[:], b.orientation[:]))
        elif b.shape == 2:
            out.append(cq.box(b.size[:], b.position[:], b.orientation[:]))
        else:
            out.append(cq.sphere(b.size[0], b.position[:]))
    return out


def static_force(orc, s, p):
    """F [n, 3] of the static world on the spheres, and whether each touches anything"""
    x, v = s["x"], s["v"]
    F = np.zeros_like(x)
    touching = np.zeros(len(x), dtype=bool)
    for b in static_bodies(orc):
        sdf, nrm, _ = cq.body_distance(b, b["position"], x, np.float64)
        depth = s["r"] - sdf
        vn = np.einsum("ni,ni->n", v, nrm)
        fn = p["contact_kp"] * depth - p["contact_kd"] * vn
        on = (depth > 0) & (fn > 0) & (s["m"] > 0)
        vt = v - vn[:, None] * nrm
        fr = p["friction"] * fn / np.sqrt(np.einsum("ni,ni->n", vt, vt) + p["slip_eps"] ** 2)
        F += np.where(on[:, None], fn[:, None] * nrm - fr[:, None] * vt, 0.0)
        touching |= on
    return F, touching


# ---- the arm's samples ----------------------------------------------------------------------------------------------------------
def samples_world(orc):
    """[(body, c, radius, position [n, 3], velocity [n, 3], R_b [n, 3, 3])] of the arm's active contact samples at the oracle's
    joints: the pointer's sample always, all 23 with link_contacts (DynOracle.contact_samples)."""
    q, qd = orc.dstate["q"], orc.dstate["qd"]
    R, o, v, w = lk.link_frames(q, qd)
    links = ext.body_links()
    out = []
    for body, c, radius in orc.contact_samples():
        radius = radius if radius >= 0 else float(orc.d.pointer_radius)        # (the oracle's table marks the pointer's with -1)
        k = links[body]
        rc = np.einsum("nij,j->ni", R[:, k], c)
        out.append((body, c, radius, o[:, k] + rc, v[:, k] + np.cross(w[:, k], rc), R[:, k]))
    return out


def arm_forces(orc, s, p):
    """(F [n, 3] of the arm's samples on the spheres, fext [n, 6, 6] of the reactions on the arm's bodies (n_b | f_b, body
    coordinates), touching [n])"""
    n = orc.n
    F, fext, touching = np.zeros((n, 3)), np.zeros((n, DOF, 6)), np.zeros(n, dtype=bool)
    for body, c, radius, pos, vel, Rb in samples_world(orc):
        d = s["x"] - pos
        length = np.linalg.norm(d, axis=1)
        nrm = np.where((length > 0)[:, None], d / np.where(length > 0, length, 1.0)[:, None], np.array([0.0, 0.0, 1.0]))
        depth = s["r"] + radius - length
        fn = p["contact_kp"] * depth - p["contact_kd"] * np.einsum("ni,ni->n", s["v"] - vel, nrm)
        on = (depth > 0) & (fn > 0) & (s["m"] > 0)
        f = np.where(on[:, None], fn[:, None] * nrm, 0.0)
        F += f
        fb = np.einsum("nji,nj->ni", Rb, -f)                           # R_b^T (-f): the reaction in body coordinates
        fext[:, body, 0:3] += np.cross(c, fb)
        fext[:, body, 3:6] += fb
        touching |= on
    return F, fext, touching


def integrate(s, F, p, g, h):
    """the spheres' sub-step under the force F [n, 3] (static world plus arm), in place on s; an env without a sphere stays as it is"""
    live = s["m"] > 0
    inv_m = np.where(live, 1.0 / np.where(live, s["m"], 1.0), 0.0)
    acc = F * inv_m[:, None] - p["linear_damping"] * s["v"] - np.array([0.0, 0.0, g])
    vn = s["v"] + h * acc
    s["v"] = np.where(live[:, None], vn, s["v"])
    s["x"] = np.where(live[:, None], s["x"] + h * vn, s["x"])
