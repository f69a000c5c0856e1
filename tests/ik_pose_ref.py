"""Independent float64 reference of pnr_solve_ik_pose and the input sets its CPU and GPU tests share.

Built on tests/ik_ref.py (jacobian) and tests/link_kinematics_ref.py (link_frames) alone; it reads nothing of pioneer_amd.

The law of include/pioneer_amd.h, per env:
    q = clamp(q_init, r_lo, r_hi)
    repeat up to max_iterations times:
        e_p = target_pos - p(q)
        (s, c) = the sine vector and cosine of the rotation still to make:
            FULL: s = 1/2 sum_k r_k x t_k, c = (sum_k r_k . t_k - 1) / 2      (r_k, t_k: columns of R(q), R_target)
            AXIS: s = u x v, c = u . v                                          (u = R(q) a, v = R_target a)
        angle = atan2(|s|, c);  e_o = s * angle / max(|s|, 1e-12)
        stop (frozen from now on) if |e_p| <= tolerance and angle <= angle_tolerance
        e = [e_p ; w e_o];  J = [J_lin ; w J_ang]
        lambda^2 = damping^2 + error_damping * (|e_p|^2 + w^2 angle^2)
        y = (J J^T + lambda^2 I)^-1 e
        dq = J^T y;  dq *= min(1, max_step / max_j |dq_j|)
        q = clamp(q + dq, r_lo, r_hi)
In FULL mode s is the vector of the antisymmetric part of R_target R(q)^T, so e_o is that rotation's rotation vector.  Where the
axis cannot be formed (half a turn, opposite vectors: |s| = 0, c < 0) the max() makes the orientation step zero (finite) while
`angle` stays pi.

`dtype=np.float32` gives the float32 emulation of the law: a second correct float32 implementation, whose distance from the
float64 law measures what float32 rounding alone does to the joints.  kinematics_f32 (lk.link_frames in float32) rounds every
link's rotation and position, the sines and cosines, the Jacobian and the error to float32, the target's rotation is formed in
float32 from the float32 quaternion (lk.matrix_from_quat in float32); the system, its solve and the update run in float32 (numpy's
float32 matmul and LAPACK's sgesv).  The float64 law itself uses ik_ref.jacobian and lk.link_frames only.
"""
import numpy as np

import ik_ref
import link_kinematics_ref as lk

FULL, AXIS = 0, 1
DEFAULTS = dict(max_iterations=32, damping=0.03, error_damping=0.01, orientation_weight=10.0, max_step=0.5, tolerance=1e-3,
                angle_tolerance=1e-3)
LIMITS = np.array([3.1416, 1.309, 1.309, 3.1416, 1.5708, 3.1416])
INNER_LO, INNER_HI = np.array([15.0, -8.0, 2.0]), np.array([22.0, 8.0, 6.0])
S_FLOOR = 1e-12


def link_pose(q, link=10, local_point=None, chain=None):
    """World position of the point [N, 3] and the link's world rotation [N, 3, 3]."""
    R, p, _, _ = lk.link_frames(q, None, chain)
    local = np.zeros(3) if local_point is None else np.asarray(local_point, dtype=np.float64)
    return p[:, link] + R[:, link] @ local, R[:, link]


def orientation_error(R, R_target, mode=FULL, local_axis=(1.0, 0.0, 0.0)):
    """(e_o [N, 3] world-frame rotation vector, angle [N] in [0, pi]) from the rotations R to R_target [N, 3, 3]."""
    if mode == FULL:
        s = 0.5 * np.cross(R.transpose(0, 2, 1), R_target.transpose(0, 2, 1)).sum(axis=1)      # rows of R^T = columns of R
        c = 0.5 * ((R * R_target).sum(axis=(1, 2)) - 1.0)
    else:
        a = np.asarray(local_axis, dtype=np.float64)
        a = a / np.linalg.norm(a)
        u, v = R @ a, R_target @ a
        s, c = np.cross(u, v), (u * v).sum(axis=1)
    sn = np.linalg.norm(s, axis=1)
    angle = np.arctan2(sn, c)
    return s * (angle / np.maximum(sn, S_FLOOR))[:, None], angle


def pose_error(q, target_pos, target_quat, mode=FULL, local_axis=(1.0, 0.0, 0.0), link=10, local_point=None, chain=None):
    """(distance [N], angle [N]) of the joints q [N, 6] from the target pose, by the float64 chain."""
    p, R = link_pose(np.asarray(q, dtype=np.float64), link, local_point, chain)
    _, angle = orientation_error(R, lk.matrix_from_quat(np.atleast_2d(target_quat)), mode, local_axis)
    return np.linalg.norm(np.asarray(target_pos, dtype=np.float64) - p, axis=1), angle


def kinematics_f32(q, link=10, local_point=None, chain=None):
    """From the chain walked with float32 results at every step: (point [N, 3], R of the link [N, 3, 3], J [N, 6, 6]) in float32."""
    f = np.float32
    q = np.atleast_2d(np.asarray(q, dtype=f))
    # (with qdd the walk hands out the joints' world axes as it forms them, before the joint's own rotation)
    R, p, _, _, _, _, axes, origins = lk.link_frames(q, chain=chain, qdd=np.zeros_like(q), dtype=f, upto=link)
    local = np.zeros(3, dtype=f) if local_point is None else np.asarray(local_point, dtype=f)
    point = p[:, link] + R[:, link] @ local
    J = np.zeros((q.shape[0], 6, 6), dtype=f)
    J[:, 0:3, :axes.shape[1]] = np.cross(axes, point[:, None] - origins).transpose(0, 2, 1)
    J[:, 3:6, :axes.shape[1]] = axes.transpose(0, 2, 1)
    assert point.dtype == R.dtype == J.dtype == f
    return point, R[:, link], J


def solve_ik_pose(target_pos, target_quat, q_init=None, link=10, local_point=None, mode=FULL, local_axis=(1.0, 0.0, 0.0),
                  max_iterations=32, damping=0.03, error_damping=0.01, orientation_weight=10.0, max_step=0.5, tolerance=1e-3,
                  angle_tolerance=1e-3, chain=None, dtype=np.float64):
    """Returns (q [N, 6], residual [N], angle [N], iterations [N] int).  Limits: the float32 limits of the engine."""
    chain = chain or lk.load_chain()
    target_pos = np.atleast_2d(np.asarray(target_pos, dtype=np.float64))
    Rt = lk.matrix_from_quat(np.atleast_2d(target_quat), dtype).astype(np.float64)
    n = target_pos.shape[0]
    lo, hi = (v.astype(dtype) for v in ik_ref.limits_f32(chain))
    q = np.zeros((n, 6)) if q_init is None else np.array(np.broadcast_to(np.asarray(q_init, dtype=np.float64), (n, 6)))
    q = np.clip(q.astype(dtype), lo, hi)
    w = float(orientation_weight)
    frozen = np.zeros(n, dtype=bool)
    iters = np.zeros(n, dtype=np.int64)
    eye = np.eye(6, dtype=dtype)[None]
    for _ in range(int(max_iterations)):
        if dtype is np.float32:
            p, R, J = kinematics_f32(q, link, local_point, chain)
            p, R = p.astype(np.float64), R.astype(np.float64)
        else:
            p, R = link_pose(q, link, local_point, chain)
        e_p = target_pos - p
        e_o, angle = orientation_error(R, Rt, mode, local_axis)
        dist = np.linalg.norm(e_p, axis=1)
        frozen |= (dist <= tolerance) & (angle <= angle_tolerance)
        if frozen.all():
            break
        if dtype is not np.float32:
            J = ik_ref.jacobian(q, link, local_point, chain)
        J[:, 3:6] *= dtype(w)
        e = np.concatenate([e_p, w * e_o], axis=1).astype(dtype)
        lam2 = (damping * damping + error_damping * (dist * dist + w * w * angle * angle)).astype(dtype)
        A = J @ J.transpose(0, 2, 1) + lam2[:, None, None] * eye
        with np.errstate(invalid="ignore"):
            y = np.linalg.solve(A, e[:, :, None]) if np.isfinite(A).all() else _solve_each(A, e)
        dq = (J.transpose(0, 2, 1) @ y)[:, :, 0]
        big = np.abs(dq).max(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            scale = np.where(big > max_step, dtype(max_step) / big, dtype(1.0)).astype(dtype)
        qn = np.clip(q + dq * scale[:, None], lo, hi)
        q = np.where(frozen[:, None], q, qn).astype(dtype)
        iters += ~frozen
    dist, angle = pose_error(q, target_pos, target_quat, mode, local_axis, link, local_point, chain)
    return q.astype(np.float64), dist, angle, iters


def _solve_each(A, e):
    """np.linalg.solve env by env: an env with a non-finite system gets NaN and does not disturb the others."""
    y = np.full(e.shape + (1,), np.nan, dtype=A.dtype)
    for k in range(A.shape[0]):
        if np.isfinite(A[k]).all() and np.isfinite(e[k]).all():
            y[k] = np.linalg.solve(A[k], e[k][:, None])
    return y


def fk_pose(q, link=10, local_point=None):
    """(position [N, 3], quaternion (x, y, z, w) [N, 4]) of the link at the joints q, float64."""
    p, R = link_pose(q, link, local_point)
    return p, lk.quat_from_matrix(R)


def near_set(n, seed):
    """NEAR: q_t = U(-0.8, 0.8) limits with q_t[4] = +-U(0.4, 1.2) (away from the wrist singularity q5 = 0), the target its
    FK pose, the start q_t + U(-0.2, 0.2) per joint.  Returns float32 (target_pos [n, 3], target_quat [n, 4], start [n, 6])
    and q_t: what both the engine and the reference are given."""
    rng = np.random.default_rng(seed)
    q_t = rng.uniform(-0.8, 0.8, size=(n, 6)) * LIMITS
    q_t[:, 4] = rng.choice([-1.0, 1.0], size=n) * rng.uniform(0.4, 1.2, size=n)
    start = q_t + rng.uniform(-0.2, 0.2, size=(n, 6))
    pos, quat = fk_pose(q_t)
    return pos.astype(np.float32), quat.astype(np.float32), start.astype(np.float32), q_t


def point_set(n, seed):
    """POINT: positions uniform in the inner box, the pointer's local x axis along world +x with a random roll about it (which
    AXIS mode must ignore); solved in AXIS mode with local_axis (1, 0, 0) from the rest pose.  float32 (pos, quat)."""
    rng = np.random.default_rng(seed)
    pos = INNER_LO + (INNER_HI - INNER_LO) * rng.random((n, 3))
    roll = rng.uniform(-np.pi, np.pi, size=n)
    quat = np.stack([np.sin(roll / 2), np.zeros(n), np.zeros(n), np.cos(roll / 2)], axis=1)
    return pos.astype(np.float32), quat.astype(np.float32)


def fk_set(n, seed, lo=0.8, hi=0.9):
    """FK poses of random joints inside U(lo, hi)-scaled limits, for rest-pose starts: float32 (pos, quat) and the joints."""
    rng = np.random.default_rng(seed)
    q_t = rng.uniform(-1.0, 1.0, size=(n, 6)) * rng.uniform(lo, hi, size=(n, 1)) * LIMITS
    pos, quat = fk_pose(q_t)
    return pos.astype(np.float32), quat.astype(np.float32), q_t


def law_cases():
    """The fixed-iteration cases of the law-parity tests: (name, iterations, mode, start given?)."""
    return [(f"{its} iteration{'s' if its > 1 else ''}, {'AXIS' if mode else 'FULL'}, {'NEAR' if near else 'rest'} start", its, mode, near)
            for its, near in ((1, True), (3, True), (1, False)) for mode in (FULL, AXIS)]


LAW_PARAMS = dict(damping=0.1, error_damping=0.01, tolerance=0.0, angle_tolerance=0.0)     # the better-conditioned setting
MAX_START_ANGLE = 3.0      # rad: towards half a turn the rotation axis is ill-conditioned in any number format
_law_cache = {}


def law_reference(n, iterations, mode, near):
    """The law-parity inputs at n envs and what the float64 law and its float32 emulation make of them: (pos, quat, start or
    None, q64, q32, held); computed once per case.  held [n] bool: the envs whose start is less than MAX_START_ANGLE from the
    target's orientation, whose joints are compared (every NEAR start; from the rest pose all but the poses that are
    nearly half a turn away, 9-12 % in FULL mode, where forming R_target in float32 alone moves the first step by up to 6e-5 rad)."""
    key = (n, iterations, mode, near)
    if key not in _law_cache:
        pos, quat, start, _ = near_set(n, NEAR_SEED(n))
        start = start if near else None
        kw = dict(LAW_PARAMS, max_iterations=iterations, mode=mode)
        q64 = solve_ik_pose(pos, quat, start, **kw)[0]
        q32 = solve_ik_pose(pos, quat, start, dtype=np.float32, **kw)[0]
        held = pose_error(np.zeros((n, 6)) if start is None else start, pos, quat, mode)[1] < MAX_START_ANGLE
        _law_cache[key] = (pos, quat, start, q64, q32, held)
    return _law_cache[key]


def law_deviation(iterations, mode, near):
    """Largest joint distance (rad) between the float32 emulation and the float64 law over the held envs of the NEAR sets of
    every size in SIZES, for one case: the deviation a correct float32 implementation shows on these inputs."""
    return max(float(np.abs(r[3] - r[4])[r[5]].max()) for r in (law_reference(n, iterations, mode, near) for n in SIZES))


# the sizes and seeds the GPU tests use (tests/test_gpu_ik_pose.py); tests/test_ik_pose_cpu.py proves that the reference converges
# for every env of each
SIZES = [1, 37, 64, 1000]
NEAR_SEED = lambda n: 300 + n    # noqa: E731
POINT_SEED = lambda n: 400 + n   # noqa: E731
