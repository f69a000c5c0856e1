"""Independent float64 reference of pnr_get_jacobian and pnr_solve_ik.

Built on tests/link_kinematics_ref.py and tests/golden/urdf_chain.json alone; it reads nothing of pioneer_amd.

Jacobian of link k at a point fixed in the link's frame: column j (revolute joints in URDF order) is a_j x (point - o_j)
for the linear rows and a_j for the angular rows, a_j the joint's world axis and o_j its world origin; joints that are not
between the base and the link have zero columns.

Solver: the damped-least-squares law of include/pioneer_amd.h, per env:
    q = clamp(q_init, r_lo, r_hi)
    repeat up to max_iterations times:
        e = target - p(q);  stop (frozen from now on) if |e| <= tolerance
        J = the three linear rows of the Jacobian at q
        y = (J J^T + lambda^2 I)^-1 e
        dq = J^T y;  dq *= min(1, max_step / max_j |dq_j|)
        q = clamp(q + dq, r_lo, r_hi)
"""
import numpy as np

import link_kinematics_ref as lk

NUM_LINKS = 11
DOF = 6


def revolute_links(chain=None):
    """Link index (= URDF joint index) of each revolute joint, axis [6, 3], and the limits (lower, upper) [6] each."""
    chain = chain or lk.load_chain()
    idx = [k for k, j in enumerate(chain) if j["type"] == "revolute"]
    axes = np.array([chain[k]["axis"] for k in idx], dtype=np.float64)
    lo = np.array([chain[k]["lower"] for k in idx], dtype=np.float64)
    hi = np.array([chain[k]["upper"] for k in idx], dtype=np.float64)
    return idx, axes, lo, hi


def limits_f32(chain=None):
    """The joint limits as the engine holds them: float32 of the URDF's numbers."""
    _, _, lo, hi = revolute_links(chain)
    return lo.astype(np.float32), hi.astype(np.float32)


def point_position(q, link=10, local_point=None, chain=None):
    """World position [N, 3] of the point `local_point` of link `link`."""
    R, p, _, _ = lk.link_frames(q, None, chain)
    local = np.zeros(3) if local_point is None else np.asarray(local_point, dtype=np.float64)
    return p[:, link] + R[:, link] @ local


def jacobian(q, link=10, local_point=None, chain=None):
    """[N, 6, 6] float64: rows 0-2 linear, rows 3-5 angular, column j = revolute joint j."""
    chain = chain or lk.load_chain()
    q = np.atleast_2d(np.asarray(q, dtype=np.float64))
    R, p, _, _ = lk.link_frames(q, None, chain)
    idx, axes, _, _ = revolute_links(chain)
    local = np.zeros(3) if local_point is None else np.asarray(local_point, dtype=np.float64)
    point = p[:, link] + R[:, link] @ local
    J = np.zeros((q.shape[0], 6, DOF))
    for j, (k, axis) in enumerate(zip(idx, axes)):
        if k > link:                    # a serial chain: joint k's child is link k, upstream of every later link
            continue
        a = R[:, k] @ axis
        J[:, 0:3, j] = np.cross(a, point - p[:, k])
        J[:, 3:6, j] = a
    return J


def solve_ik(target, q_init=None, link=10, local_point=None, max_iterations=32, damping=1.0, max_step=0.5, tolerance=1e-3,
             chain=None):
    """Returns (q [N, 6], residual [N], iterations [N] int) in float64.  Limits: the float32 limits of the engine."""
    chain = chain or lk.load_chain()
    target = np.atleast_2d(np.asarray(target, dtype=np.float64))
    n = target.shape[0]
    lo, hi = (v.astype(np.float64) for v in limits_f32(chain))
    q = np.zeros((n, DOF)) if q_init is None else np.array(np.broadcast_to(np.asarray(q_init, dtype=np.float64), (n, DOF)))
    q = np.clip(q, lo, hi)
    frozen = np.zeros(n, dtype=bool)
    iters = np.zeros(n, dtype=np.int64)
    eye = np.eye(3)[None]
    for _ in range(int(max_iterations)):
        e = target - point_position(q, link, local_point, chain)
        frozen |= np.linalg.norm(e, axis=1) <= tolerance
        if frozen.all():
            break
        J = jacobian(q, link, local_point, chain)[:, 0:3]
        A = J @ J.transpose(0, 2, 1) + damping * damping * eye
        y = np.linalg.solve(A, e[:, :, None])
        dq = (J.transpose(0, 2, 1) @ y)[:, :, 0]
        big = np.abs(dq).max(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            scale = np.where(big > max_step, max_step / big, 1.0)
        qn = np.clip(q + dq * scale[:, None], lo, hi)
        q = np.where(frozen[:, None], q, qn)
        iters += ~frozen
    residual = np.linalg.norm(target - point_position(q, link, local_point, chain), axis=1)
    return q, residual, iters
