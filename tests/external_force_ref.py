"""Independent float64 reference of pnr_world_step_wrenches (external forces and torques on links of the arm).

The law is the one stated in include/pioneer_amd.h.  One call is frame_skip sub-steps of length h.  A record is (link, frame)
plus, per env, force[3] | position[3] | torque[3].  The link maps to its dynamic body b (the revolute joints up to the link,
fixed joints merged) and to the link origin's fixed offset d in body coordinates.
    frame "link":   f_b = force,  n_b = (d + position) x force + torque,  constant over the call
    frame "world":  p_b = R_b(q0)^T (position - o_b(q0)) at the call's first pose, then in every sub-step
                    f_b = R_b(q_k)^T force,  n_b = p_b x f_b + R_b(q_k)^T torque
    fext[b] += (n_b, f_b) in the first `hold` sub-steps, on top of the contact wrenches; link 0 (the welded base) does nothing.

This module turns the records into fext (`prepare` once per call, `body_wrenches` per sub-step); the sub-step that takes fext is
tests/world_step_ref.py's, whose world_step(wrenches=(specs, w), hold_substeps=...) is the reference of the call.  The poses R_b,
o_b and the link offsets come from tests/link_kinematics_ref.py (the URDF chain of tests/golden/urdf_chain.json), not from the
oracle or the engine.  It reads nothing of pioneer_amd.
"""
import numpy as np

import ik_ref
import link_kinematics_ref as lk

DOF = 6
NUM_LINKS = 11


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
