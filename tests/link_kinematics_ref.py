"""Independent reference of pnr_get_link_states: world pose and velocity of every URDF link; and the one walk over the URDF chain
that every reference under tests/ poses the arm with (`link_frames`), with the one quaternion -> matrix (`matrix_from_quat`).

It reads tests/golden/urdf_chain.json (the URDF's numbers) alone: not the engine, its model table or pioneer_amd.  Link k is the
child of URDF joint k (Bullet's link_index), so links come out in the order
robot:base, rotator1, hinge1, arm1, arm2, rotator2, hinge2, arm3, rotator3, effector, pointer.

Record layout (13 floats per link): position[3], quaternion (x, y, z, w) with w >= 0, linear velocity of the link frame
origin[3], angular velocity[3], all in the world frame.
"""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "urdf_chain.json")


def load_chain(path=GOLDEN):
    with open(path) as f:
        return json.load(f)["joints"]


# Two forms of the joint rotation, chosen by link_frames' caller: in float32 they differ by an ulp and the *_FLOOR constants sit within 2 % of
# their floors (Rodrigues in the contact reference: distance 3.95e-6 -> 4.37e-6 > DIST_FLOOR 4.2e-6; entry-wise in the others: 7.43e-3 > 7.2e-3).
def axis_rotation(axis, q, dtype=np.float64):
    """Rotation matrices [N, 3, 3] about the unit axis by the angles q [N] (Rodrigues: I + s K + (1 - c) K^2), in `dtype`."""
    T = np.dtype(dtype).type
    a = np.asarray(axis, dtype=T)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=T)
    q = np.asarray(q, dtype=T)
    s, c = np.sin(q)[:, None, None], np.cos(q)[:, None, None]
    return np.eye(3, dtype=T)[None] + s * K[None] + (T(1) - c) * (K @ K)[None]


def coordinate_rotation(axis, q, dtype=np.float64):
    """axis_rotation about +- a coordinate axis (asserted), written entry by entry: 1, c, -+s."""
    T = np.dtype(dtype).type
    axis, q = np.asarray(axis, dtype=T), np.asarray(q, dtype=T)
    k = int(np.argmax(np.abs(axis)))
    assert abs(axis[k]) == 1.0 and np.count_nonzero(axis) == 1
    a, b = (k + 1) % 3, (k + 2) % 3
    c, s = np.cos(q), np.sin(q) * T(axis[k])
    R = np.zeros((q.shape[0], 3, 3), dtype=T)
    R[:, k, k] = 1
    R[:, a, a] = c; R[:, a, b] = -s; R[:, b, a] = s; R[:, b, b] = c
    return R


def rpy_rotation(rpy):
    """URDF <origin rpy>: R = Rz(yaw) Ry(pitch) Rx(roll)."""
    r, p, y = (float(v) for v in rpy)
    one = np.ones(1)
    return (axis_rotation((0, 0, 1), y * one) @ axis_rotation((0, 1, 0), p * one) @ axis_rotation((1, 0, 0), r * one))[0]


def quat_from_matrix(R):
    """Unit quaternions (x, y, z, w) [N, 4] of rotation matrices [N, 3, 3] (Shepperd: the largest of w, x, y, z is formed
    from the diagonal), made canonical with w >= 0."""
    R = np.asarray(R, dtype=np.float64)
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    cand = np.stack([tr, R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]], axis=1)
    k = np.argmax(cand, axis=1)
    m = lambda i, j: R[:, i, j]  # noqa: E731
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):   # the forms not picked may blow up
        forms = []
        s = 2.0 * np.sqrt(np.maximum(1.0 + tr, 1e-300))
        forms.append([(m(2, 1) - m(1, 2)) / s, (m(0, 2) - m(2, 0)) / s, (m(1, 0) - m(0, 1)) / s, 0.25 * s])
        s = 2.0 * np.sqrt(np.maximum(1.0 + m(0, 0) - m(1, 1) - m(2, 2), 1e-300))
        forms.append([0.25 * s, (m(0, 1) + m(1, 0)) / s, (m(0, 2) + m(2, 0)) / s, (m(2, 1) - m(1, 2)) / s])
        s = 2.0 * np.sqrt(np.maximum(1.0 + m(1, 1) - m(0, 0) - m(2, 2), 1e-300))
        forms.append([(m(0, 1) + m(1, 0)) / s, 0.25 * s, (m(1, 2) + m(2, 1)) / s, (m(0, 2) - m(2, 0)) / s])
        s = 2.0 * np.sqrt(np.maximum(1.0 + m(2, 2) - m(0, 0) - m(1, 1), 1e-300))
        forms.append([(m(0, 2) + m(2, 0)) / s, (m(1, 2) + m(2, 1)) / s, 0.25 * s, (m(1, 0) - m(0, 1)) / s])
        forms = np.stack([np.stack(f, axis=1) for f in forms], axis=0)  # [4 forms, N, 4]
    q = forms[k, np.arange(R.shape[0])]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[q[:, 3] < 0] *= -1.0
    return q


def matrix_from_quat(quat, dtype=np.float64):
    """Rotation matrices [N, 3, 3] (or [3, 3]) of quaternions (x, y, z, w) [N, 4] (or [4]): normalised here and formed in `dtype`;
    the sign of w does not matter."""
    T = np.dtype(dtype).type
    quat = np.asarray(quat, dtype=T)
    quat = quat / np.sqrt((quat * quat).sum(axis=-1, keepdims=True, dtype=T))
    x, y, z, w = (quat[..., i] for i in range(4))
    one, two = T(1), T(2)
    R = np.stack([
        np.stack([one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)], axis=-1),
        np.stack([two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)], axis=-1),
        np.stack([two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)], axis=-1)], axis=-2)
    assert R.dtype == np.dtype(dtype)
    return R


def link_frames(q, qd=None, chain=None, *, qdd=None, gravity=0.0, dtype=np.float64, rotation=axis_rotation, upto=None):
    """The walk over the chain (parent -> xyz -> rpy -> joint rotation -> child), forward kinematics and velocity sweep, every
    array in `dtype` at every step.  q, qd [N, 6] (revolute joints in URDF order); `rotation`: axis_rotation or
    coordinate_rotation; `upto`: the last link to visit.  Returns per link (R [N, L, 3, 3], p [N, L, 3], v [N, L, 3], w [N, L, 3]).
    With qdd [N, 6] the acceleration sweep too (gravity as the base's acceleration +g z): per link the angular acceleration and the
    origin's linear acceleration [N, L, 3], per revolute joint the world axis and origin [N, J, 3]."""
    T = np.dtype(dtype).type
    chain = chain or load_chain()
    q = np.atleast_2d(np.asarray(q, dtype=T))
    n = q.shape[0]
    qd = np.zeros_like(q) if qd is None else np.atleast_2d(np.asarray(qd, dtype=T))
    zero = np.zeros((n, 3), dtype=T)
    g0 = zero.copy()
    g0[:, 2] = T(gravity)
    if qdd is not None:
        qdd = np.atleast_2d(np.asarray(qdd, dtype=T))
    frames = {"world": (np.broadcast_to(np.eye(3, dtype=T), (n, 3, 3)), zero, zero, zero, zero, g0)}
    links, joints, qi = [], [], 0
    for j in chain[:None if upto is None else upto + 1]:
        Rp, pp, vp, wp, alp, accp = frames[j["parent"]]
        d = Rp @ np.asarray(j["xyz"], dtype=T)
        p = pp + d
        R = Rp @ rpy_rotation(j["rpy"]).astype(T)
        v = vp + np.cross(wp, p - pp)
        w, al, acc = wp, alp, accp
        if qdd is not None:
            acc = accp + np.cross(alp, d) + np.cross(wp, np.cross(wp, d))
        if j["type"] == "revolute":
            axis = np.asarray(j["axis"], dtype=T)
            a = R @ axis
            w = wp + qd[:, qi:qi + 1] * a
            if qdd is not None:
                al = alp + qdd[:, qi:qi + 1] * a + qd[:, qi:qi + 1] * np.cross(wp, a)
            R = R @ rotation(axis, q[:, qi], T)
            joints.append((a, p))
            qi += 1
        else:
            assert j["type"] == "fixed", j["type"]
        frames[j["child"]] = (R, p, v, w, al, acc)
        links.append(frames[j["child"]])
    assert all(x.dtype == np.dtype(dtype) for fr in links for x in fr)
    out = tuple(np.stack([fr[i] for fr in links], axis=1) for i in range(4 if qdd is None else 6))
    return out if qdd is None else out + tuple(np.stack([jt[i] for jt in joints], axis=1) for i in range(2))


def link_states(q, qd, chain=None):
    """The [N, 11, 13] float64 records pnr_get_link_states writes."""
    R, p, v, w = link_frames(q, qd, chain)
    n, L = p.shape[:2]
    quat = quat_from_matrix(R.reshape(n * L, 3, 3)).reshape(n, L, 4)
    return np.concatenate([p, quat, v, w], axis=2)
