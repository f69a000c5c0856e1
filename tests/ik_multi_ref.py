"""Independent float64 reference of pnr_solve_ik_multi and the input sets its CPU and GPU tests share.

Built on tests/ik_ref.py (solve_ik) and tests/ik_pose_ref.py (solve_ik_pose) alone; it reads nothing of pioneer_amd.

Every start is one solve of the single-start reference (the S starts of the n envs go through it as n S independent rows: a
row's result does not depend on the rows around it).  A start is converged when the pose it ends at is within the tolerances.
Per env the winner is the smallest (not converged, cost, start index): cost = sum_j (q_j - q_ref_j)^2 for a converged start
(q_ref None: the env's clamped start 0), |e_p| + w angle for the others (the position task: |e_p|); a cost that is not finite
counts as +inf.  Policy BEST: every start runs to its end.  Policy FIRST: the env stops at the first convergence check in which
one of its starts is converged, i.e. every start makes at most k* iterations, k* the fewest iterations of a converged start.
"""
import numpy as np

import ik_pose_ref as pref
import ik_ref

POSITION, POSE, AXIS = 0, 1, 2
BEST, FIRST = 0, 1
LIMITS = pref.LIMITS
POSITION_DEFAULTS = dict(max_iterations=32, damping=1.0, max_step=0.5, tolerance=1e-3)
BOX_LO, BOX_HI = np.array([15.0, -10.0, 2.0]), np.array([25.0, 10.0, 6.0])     # the reference's own target box

# the sets the CPU and the GPU tests share
FULL_SET = (1000, 11)            # pref.fk_set(n, seed): full poses of random joints at 0.8-0.9 of the limits
TABLE_SEED = 0                   # the default table's seed
BOX_SEED = 61


def start_table(S, seed=TABLE_SEED):
    """The default table: row 0 the rest pose, the others U(-0.8, 0.8) LIMITS from default_rng(seed), drawn row by row; float32."""
    table = np.random.default_rng(int(seed)).uniform(-0.8, 0.8, size=(int(S), 6)) * LIMITS
    table[0] = 0.0
    return table.astype(np.float32)


def box_targets(n, seed=BOX_SEED):
    return (BOX_LO + (BOX_HI - BOX_LO) * np.random.default_rng(seed).random((n, 3))).astype(np.float32)


def clamp(q):
    lo, hi = (v.astype(np.float64) for v in ik_ref.limits_f32())
    return np.clip(np.asarray(q, dtype=np.float64), lo, hi)


def env_starts(n, table, q_init=None):
    """[n, S, 6] float64: the starts of every env as given (table [S, 6] or [n, S, 6]; q_init [n, 6] replaces start 0)."""
    table = np.asarray(table, dtype=np.float64)
    st = np.array(np.broadcast_to(table, (n,) + table.shape[-2:]))
    if q_init is not None:
        st[:, 0] = np.asarray(q_init, dtype=np.float64)
    return st


def solve_rows(task, pos, quat, start, local_axis=(1.0, 0.0, 0.0), **kw):
    """The single-start reference on rows: (q, residual, angle, iterations); the position task's angle is 0."""
    if task == POSITION:
        kw = {k: v for k, v in kw.items() if k not in ("error_damping", "orientation_weight", "angle_tolerance")}
        q, res, its = ik_ref.solve_ik(pos, start, **kw)
        return q, res, np.zeros_like(res), its
    return pref.solve_ik_pose(pos, quat, start, mode=pref.AXIS if task == AXIS else pref.FULL, local_axis=local_axis, **kw)


def is_converged(task, res, ang, kw):
    tol = kw.get("tolerance", 1e-3)
    return res <= tol if task == POSITION else (res <= tol) & (ang <= kw.get("angle_tolerance", 1e-3))


def solve_starts(task, pos, quat, table, q_init=None, **kw):
    """Every start of every env to its end: dict of all_q [n, S, 6], all_residual, all_angle, all_iterations, converged [n, S]."""
    pos = np.atleast_2d(np.asarray(pos, dtype=np.float64))
    n = pos.shape[0]
    st = env_starts(n, table, q_init)
    S = st.shape[1]
    rep = lambda a: None if a is None else np.repeat(np.asarray(a, dtype=np.float64), S, axis=0)  # noqa: E731
    q, res, ang, its = solve_rows(task, rep(pos), rep(quat), st.reshape(n * S, 6), **kw)
    out = dict(all_q=q.reshape(n, S, 6), all_residual=res.reshape(n, S), all_angle=ang.reshape(n, S), all_iterations=its.reshape(n, S))
    out["converged_starts"] = is_converged(task, out["all_residual"], out["all_angle"], kw)
    return out


def costs(task, all_q, all_residual, all_angle, conv, q_ref, weight):
    """[n, S]: the selection's cost of every start; not finite -> +inf."""
    near = ((all_q - q_ref[:, None, :]) ** 2).sum(axis=2)
    left = all_residual + (0.0 if task == POSITION else weight) * all_angle
    cost = np.where(conv, near, left)
    return np.where(np.isfinite(cost), cost, np.inf)


def select(task, per, q_ref, weight):
    """The winner's start index [n] by the key (not converged, cost, index)."""
    conv = per["converged_starts"]
    cost = costs(task, per["all_q"], per["all_residual"], per["all_angle"], conv, q_ref, weight)
    n, S = cost.shape
    order = np.lexsort((np.broadcast_to(np.arange(S), (n, S)), cost, ~conv), axis=1)      # last key first
    return order[:, 0]


def solve_multi(task, pos, quat, table, q_init=None, q_ref=None, policy=BEST, **kw):
    """dict: the winner's q [n, 6], residual, angle, iterations, start, converged (count) and the per-start fields."""
    pos = np.atleast_2d(np.asarray(pos, dtype=np.float64))
    n = pos.shape[0]
    per = solve_starts(task, pos, quat, table, q_init, **kw)
    if policy == FIRST:
        max_it = kw.get("max_iterations", 32)
        its = np.where(per["converged_starts"], per["all_iterations"], np.iinfo(np.int64).max)
        kstar = its.min(axis=1)                                                   # the check in which the env's first start converges
        st = env_starts(n, table, q_init)
        for k in np.unique(kstar[kstar < max_it]):
            rows = np.nonzero(kstar == k)[0]
            sub = solve_starts(task, pos[rows], None if quat is None else np.asarray(quat)[rows], st[rows], **dict(kw, max_iterations=int(k)))
            for key in per:
                per[key][rows] = sub[key]
    ref = clamp(env_starts(n, table, q_init)[:, 0]) if q_ref is None else np.asarray(q_ref, dtype=np.float64)
    win = select(task, per, ref, kw.get("orientation_weight", 10.0))
    take = lambda a: a[np.arange(n), win]  # noqa: E731
    return dict(per, q=take(per["all_q"]), residual=take(per["all_residual"]), angle=take(per["all_angle"]),
                iterations=take(per["all_iterations"]), start=win, converged=per["converged_starts"].sum(axis=1))


_cache = {}


def full_set_reference(S):
    """(pos, quat, q_t, per-start results of the float64 reference) of the FULL set with the default table of S starts; computed once.
    The table of S starts is the first S rows of the 16-start table, so one 16-start solve serves every S <= 16."""
    if "full" not in _cache:
        pos, quat, q_t = pref.fk_set(*FULL_SET)
        _cache["full"] = (pos, quat, q_t, solve_starts(POSE, pos, quat, start_table(16)))
    pos, quat, q_t, per = _cache["full"]
    assert S <= 16
    return pos, quat, q_t, {k: v[:, :S] for k, v in per.items()}


def box_reference(S=8, n=1000):
    """(targets, per-start results) of the position task on the full target box with the default table of S starts; computed once."""
    key = ("box", S, n)
    if key not in _cache:
        tgt = box_targets(n)
        _cache[key] = (tgt, solve_starts(POSITION, tgt, None, start_table(S), **POSITION_DEFAULTS))
    return _cache[key]
