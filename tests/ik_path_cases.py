"""The inputs the CPU and the GPU tests of pnr_solve_ik_path share: sizes, shapes, seeds and the four input families.  Everything
handed out is float32, what both the engine and the reference are given.  It reads nothing of pioneer_amd.

Families (case(family, n, K)): waypoints of K poses per env, the task, and the start that is start 0 (None: the rest pose).
  LINE   position task: every waypoint uniform in the inner box (15, -8, 2)..(22, 8, 6); from the rest pose.
  HOLD   pose task: ik_pose_ref.near_set poses and starts; the orientation held, the position moved L along a random unit direction
         per segment.
  TURN   pose task: from the FK pose of near_set's q_t to the FK pose of q_t + U(-0.3, 0.3) per joint (clamped), cumulatively.
  POINT  axis task (local x along the target's): ik_pose_ref.point_set, the position moved 2 in y towards the middle and back;
         from the rest pose.
"""
import numpy as np

import ik_multi_ref as mref
import ik_pose_ref as pref

SIZES = (1, 37, 64, 130)                    # one env, a partial wave, a full one, more than two
SHARE_ENVS = 1000                           # the tracked-share tests
# (K, M, S): the basic case; targets that are exactly the waypoints; C = 1; one env per wave (the shift edge); N = 37 crosses a wave
SHAPES = ((2, 4, 1), (3, 1, 8), (1, 8, 4), (2, 3, 64), (5, 8, 2))
FAMILIES = ("LINE", "HOLD", "TURN", "POINT")
TASK = {"LINE": mref.POSITION, "HOLD": mref.POSE, "TURN": mref.POSE, "POINT": mref.AXIS}
HOLD_LENGTHS = (1.0, 3.0)
LINE_SUBSTEPS = (4, 8)
TRACK_ITERATIONS, MAX_ITERATIONS = 8, 32
_SEED = {"LINE": 7100, "HOLD": 7200, "TURN": 7300, "POINT": 7400}


def case(family, n, K=2, length=1.0):
    """dict(task, pos [n, K, 3], quat [n, K, 4] or None, q_init [n, 6] or None), float32."""
    rng = np.random.default_rng(_SEED[family] + 13 * n + K)
    f = np.float32
    if family == "LINE":
        pos = pref.INNER_LO + (pref.INNER_HI - pref.INNER_LO) * rng.random((n, K, 3))
        return dict(task=TASK[family], pos=pos.astype(f), quat=None, q_init=None)
    if family == "POINT":
        p0, quat = pref.point_set(n, _SEED[family] + n)
        pos = np.repeat(p0[:, None].astype(np.float64), K, axis=1)
        pos[:, 1::2, 1] -= 2.0 * np.sign(p0[:, 1:2])
        return dict(task=TASK[family], pos=pos.astype(f), quat=np.repeat(quat[:, None], K, axis=1).astype(f), q_init=None)
    p0, quat0, start, q_t = pref.near_set(n, _SEED[family] + n)
    if family == "HOLD":
        d = rng.normal(size=(n, K, 3))
        d /= np.linalg.norm(d, axis=2, keepdims=True)
        d[:, 0] = 0.0
        pos = p0[:, None].astype(np.float64) + float(length) * np.cumsum(d, axis=1)
        return dict(task=TASK[family], pos=pos.astype(f), quat=np.repeat(quat0[:, None], K, axis=1).astype(f), q_init=start)
    if family == "TURN":
        q = q_t[:, None] + np.cumsum(np.concatenate([np.zeros((n, 1, 6)), rng.uniform(-0.3, 0.3, size=(n, K - 1, 6))], axis=1), axis=1)
        q = mref.clamp(q)
        pos, quat = pref.fk_pose(q.reshape(n * K, 6))
        return dict(task=TASK[family], pos=pos.reshape(n, K, 3).astype(f), quat=quat.reshape(n, K, 4).astype(f), q_init=start)
    raise KeyError(family)


def table_for(cs, S):
    """The [n, S, 6] float64 starts of a case: the default table, start 0 replaced by the case's own start."""
    n = cs["pos"].shape[0]
    return mref.env_starts(n, mref.start_table(S), cs["q_init"])
