"""Independent float64 reference of pnr_get_link_states: world pose and velocity of every URDF link.

Built from tests/golden/urdf_chain.json (the URDF's numbers) alone; it does not read the engine, its model table or
pioneer_amd.  Link k is the child of URDF joint k (Bullet's link_index), so links come out in the order
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


def axis_rotation(axis, q):
    """Rotation matrices [N, 3, 3] about the unit axis by the angles q [N] (Rodrigues)."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    s, c = np.sin(q)[:, None, None], np.cos(q)[:, None, None]
    return np.eye(3)[None] + s * K[None] + (1.0 - c) * (K @ K)[None]


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


def matrix_from_quat(q):
    x, y, z, w = (np.asarray(q, dtype=np.float64)[:, i] for i in range(4))
    return np.stack([
        np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=1),
        np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=1),
        np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)


def link_frames(q, qd=None, chain=None):
    """Forward kinematics and velocity sweep.  q, qd [N, 6] (revolute joints in URDF order).  Returns (R [N, 11, 3, 3],
    p [N, 11, 3], v [N, 11, 3], w [N, 11, 3]) in float64."""
    chain = chain or load_chain()
    q = np.atleast_2d(np.asarray(q, dtype=np.float64))
    n = q.shape[0]
    qd = np.zeros_like(q) if qd is None else np.atleast_2d(np.asarray(qd, dtype=np.float64))
    frames = {"world": (np.broadcast_to(np.eye(3), (n, 3, 3)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3)))}
    out, qi = [], 0
    for j in chain:
        Rp, pp, vp, wp = frames[j["parent"]]
        p = pp + Rp @ np.asarray(j["xyz"], dtype=np.float64)
        R = Rp @ rpy_rotation(j["rpy"])
        w = wp.copy()
        if j["type"] == "revolute":
            axis = np.asarray(j["axis"], dtype=np.float64)
            w = wp + qd[:, qi:qi + 1] * (R @ axis)
            R = R @ axis_rotation(axis, q[:, qi])
            qi += 1
        else:
            assert j["type"] == "fixed", j["type"]
        v = vp + np.cross(wp, p - pp)
        frames[j["child"]] = (R, p, v, w)
        out.append((R, p, v, w))
    return tuple(np.stack([o[i] for o in out], axis=1) for i in range(4))


def link_states(q, qd, chain=None):
    """The [N, 11, 13] float64 records pnr_get_link_states writes."""
    R, p, v, w = link_frames(q, qd, chain)
    n, L = p.shape[:2]
    quat = quat_from_matrix(R.reshape(n * L, 3, 3)).reshape(n, L, 4)
    return np.concatenate([p, quat, v, w], axis=2)
