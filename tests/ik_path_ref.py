"""Independent float64 reference of pnr_solve_ik_path.

Built on tests/ik_ref.py (solve_ik), tests/ik_pose_ref.py (solve_ik_pose and its float32 emulation) and tests/ik_multi_ref.py (the
start tables, solve_rows) alone; it reads nothing of pioneer_amd.

The law of include/pioneer_amd.h.  K waypoints and M substeps give C = 1 + (K - 1) M configurations: configuration 0 is waypoint 0,
configuration 1 + i M + (j - 1), j = 1 .. M, has the target a + u (b - a), u = (float)j / (float)M, between waypoints a = i and
b = i + 1, in float32 with every operation rounded once (`targets`, dtype float32: the stated bits; float64: the same formula
without the roundings), the orientation (1 - u) q_a + u h q_b, h = -1 where q_a . q_b < 0, normalised by whoever reads it; at j = M
the target is waypoint b itself.  Every start of every env is a row of its own: configuration c is ONE solve of the single-start
reference from the joints configuration c - 1 ended at, capped at max_iterations (c = 0) or track_iterations.  A configuration
is reached when the pose it ends at is within the tolerances; a row stops at its first configuration that is not (c_fail), and
its later entries are copies of that one with iterations 0.  A target that is not finite is not reached, with a NaN residual, and
the joints stay (the kernel's joints at such a row are whatever the clamp leaves: nothing is compared there but the verdict).
travel = sum |q_0 - q_ref| (with q_ref) + sum_{1 <= c <= c_fail} sum_j |q_c - q_(c-1)|, max_jump the largest single term of the
second sum.  Per env the winner is the smallest (not tracked, cost, start index): cost = travel for a tracked start, C - c_fail
for the others; a cost that is not finite counts as +inf.
"""
import numpy as np

import ik_multi_ref as mref
import ik_pose_ref as pref

POSITION, POSE, AXIS = mref.POSITION, mref.POSE, mref.AXIS
F = np.float32


def configurations(K, M):
    return 1 + (int(K) - 1) * int(M)


def segment_of(c, M):
    """(i, j) of configuration c: segment and step (configuration 0: (0, 0))."""
    if c == 0:
        return 0, 0
    i = (c - 1) // M
    return i, c - i * M


def targets(wp_pos, wp_quat, M, dtype=np.float32):
    """The C targets of every env from the float32 waypoints [n, K, 3] (and [n, K, 4] or None): (pos [n, C, 3], quat [n, C, 4] or
    None) in `dtype`.  float32: each operation rounded once, as stated; the quaternion is NOT normalised."""
    wp_pos = np.asarray(wp_pos, dtype=F).astype(dtype)
    wq = None if wp_quat is None else np.asarray(wp_quat, dtype=F).astype(dtype)
    n, K, _ = wp_pos.shape
    C = configurations(K, M)
    pos = np.empty((n, C, 3), dtype=dtype)
    quat = None if wq is None else np.empty((n, C, 4), dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(C):
            i, j = segment_of(c, M)
            if j == 0 or j == M:
                k = i if j == 0 else i + 1
                pos[:, c] = wp_pos[:, k]
                if wq is not None:
                    quat[:, c] = wq[:, k]
                continue
            u = dtype(F(j) / F(M)) if dtype is np.float32 else dtype(j) / dtype(M)
            a, b = wp_pos[:, i], wp_pos[:, i + 1]
            pos[:, c] = a + u * (b - a)
            if wq is not None:
                qa, qb = wq[:, i], wq[:, i + 1]
                d = qa[:, 0] * qb[:, 0]
                for k in (1, 2, 3):
                    d = d + qa[:, k] * qb[:, k]
                w = np.where(d < 0, -u, u).astype(dtype)[:, None]
                quat[:, c] = (dtype(1.0) - u) * qa + w * qb
    assert pos.dtype == dtype
    return pos, quat


def reached(task, res, ang, kw):
    return mref.is_converged(task, res, ang, kw)


def track(task, wp_pos, wp_quat, M, table, q_init=None, q_ref=None, max_iterations=32, track_iterations=8, dtype=np.float64, **kw):
    """Every start of every env along its path.  wp_pos [K, 3] or [n, K, 3] float32 (n from q_init / table / 1 when shared).
    Returns a dict: q_path [n, S, C, 6], residual, angle [n, S, C], iterations [n, S, C] int, tracked [n, S] bool, c_fail [n, S]
    int, travel, max_jump [n, S].  dtype float32 (pose and axis tasks only): the float32 emulation of the law."""
    wp_pos = np.asarray(wp_pos, dtype=F)
    n = wp_pos.shape[0] if wp_pos.ndim == 3 else (np.asarray(table).shape[0] if np.asarray(table).ndim == 3 else
                                                   (1 if q_init is None else np.asarray(q_init).shape[0]))
    wp_pos = np.broadcast_to(wp_pos, (n,) + wp_pos.shape[-2:])
    if wp_quat is not None:
        wp_quat = np.broadcast_to(np.asarray(wp_quat, dtype=F), (n,) + np.asarray(wp_quat).shape[-2:])
    st = mref.clamp(mref.env_starts(n, table, q_init))
    S = st.shape[1]
    tp, tq = targets(wp_pos, wp_quat, M)
    tp = np.repeat(tp.astype(np.float64), S, axis=0)
    tq = None if tq is None else np.repeat(tq.astype(np.float64), S, axis=0)
    R, C = n * S, tp.shape[1]
    q = st.reshape(R, 6).copy()
    out = dict(q_path=np.zeros((R, C, 6)), residual=np.zeros((R, C)), angle=np.zeros((R, C)), iterations=np.zeros((R, C), dtype=np.int64))
    stopped = np.zeros(R, dtype=bool)
    c_fail = np.full(R, -1, dtype=np.int64)
    extra = {} if dtype is np.float64 else dict(dtype=dtype)
    assert dtype is np.float64 or task != POSITION
    for c in range(C):
        if c > 0:
            for key in ("q_path", "residual", "angle"):
                out[key][:, c] = out[key][:, c - 1]                              # the copy rule; the running rows overwrite theirs
        run = ~stopped
        finite = np.isfinite(tp[:, c]).all(axis=1) & (True if tq is None else np.isfinite(tq[:, c]).all(axis=1))
        go = run & finite
        ok = np.zeros(R, dtype=bool)
        if go.any():
            cap = int(max_iterations if c == 0 else track_iterations)
            qq, res, ang, its = mref.solve_rows(task, tp[go, c], None if tq is None else tq[go, c], q[go], max_iterations=cap, **extra, **kw)
            q[go] = qq
            out["q_path"][go, c], out["residual"][go, c], out["angle"][go, c], out["iterations"][go, c] = qq, res, ang, its
            ok[go] = reached(task, res, ang, kw)
        bad = run & ~finite
        out["q_path"][bad, c], out["residual"][bad, c] = q[bad], np.nan
        c_fail[run & ~ok] = c
        stopped |= ~ok
    ref = None if q_ref is None else np.repeat(np.asarray(q_ref, dtype=np.float64), S, axis=0)
    travel, max_jump = travel_of(out["q_path"], c_fail, ref)
    out.update(tracked=~stopped, c_fail=c_fail, travel=travel, max_jump=max_jump)
    return {k: v.reshape((n, S) + v.shape[1:]) for k, v in out.items()}


def travel_of(q_path, c_fail, q_ref=None, dtype=np.float64):
    """(travel, max_jump) of rows q_path [R, C, 6] in `dtype`, accumulated one term at a time with c ascending, then j ascending,
    over the configurations up to c_fail [R] (-1: all).  float32 on the kernel's own float32 rows reproduces its order."""
    q = np.asarray(q_path).astype(dtype)
    R, C, _ = q.shape
    last = np.where(np.asarray(c_fail) < 0, C - 1, c_fail)
    travel, max_jump = np.zeros(R, dtype=dtype), np.zeros(R, dtype=dtype)
    with np.errstate(invalid="ignore"):
        if q_ref is not None:
            for j in range(6):
                travel = (travel + np.abs(q[:, 0, j] - np.asarray(q_ref).astype(dtype)[:, j])).astype(dtype)
        for c in range(1, C):
            on = c <= last
            for j in range(6):
                d = np.abs(q[:, c, j] - q[:, c - 1, j]).astype(dtype)
                travel = np.where(on, (travel + d).astype(dtype), travel)
                max_jump = np.where(on, np.fmax(max_jump, d), max_jump)
    assert travel.dtype == dtype and max_jump.dtype == dtype
    return travel, max_jump


def costs(tracked, c_fail, travel, C):
    """[n, S]: the selection's cost of every start; not finite -> +inf."""
    cost = np.where(tracked, travel, (C - c_fail).astype(np.float64))
    return np.where(np.isfinite(cost), cost, np.inf)


def select(tracked, c_fail, travel, C):
    """The winner's start index [n] by the key (not tracked, cost, index)."""
    cost = costs(tracked, c_fail, travel, C)
    n, S = cost.shape
    return np.lexsort((np.broadcast_to(np.arange(S), (n, S)), cost, ~tracked), axis=1)[:, 0]


def solve_path(task, wp_pos, wp_quat, M, table, **kw):
    """dict: the per-start fields of `track` (all_*) and the winner's: tracked, c_fail, max_residual, max_angle, travel, max_jump,
    start, tracked_starts, q_path [n, C, 6], residual, angle, iterations [n, C]."""
    per = track(task, wp_pos, wp_quat, M, table, **kw)
    n, S, C = per["residual"].shape
    win = select(per["tracked"], per["c_fail"], per["travel"], C)
    take = lambda a: a[np.arange(n), win]  # noqa: E731
    out = {"all_" + k: v for k, v in per.items()}
    out.update({k: take(v) for k, v in per.items()})
    last = np.where(out["c_fail"] < 0, C - 1, out["c_fail"])
    upto = np.arange(C)[None] <= last[:, None]
    with np.errstate(invalid="ignore"):
        out["max_residual"] = np.where(upto, out["residual"], -np.inf).max(axis=1)      # (NaN propagates: it is the largest)
        out["max_angle"] = np.where(upto, out["angle"], -np.inf).max(axis=1)
    out.update(start=win, tracked_starts=per["tracked"].sum(axis=1))
    return out
