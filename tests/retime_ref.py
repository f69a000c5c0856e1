"""Reference of pnr_retime_path and pnr_sample_trajectory: the law of include/pioneer_amd.h in numpy, in float64 or, with
dtype=np.float32, with every array in float32 (one rounding per operation, in the law's order): the "float32 floor" the GPU
tests derive their bars from.  The torque rows come from inverse_dynamics_ref.newton_euler (the world-frame Newton-Euler sweep
over the URDF links), which shares nothing with the engine's body-frame recursion.  It reads nothing of pioneer_amd.

brute_backward_step() is a second statement of ONE backward step: the set { (x, u) } of the rows, 0 <= x <= X and
0 <= x + 2u <= K_next is a bounded polygon, so max x is attained at a vertex; it enumerates the intersections of all pairs of
boundary lines and keeps the feasible ones.  tests/test_retime_cpu.py holds the pair rule against it on every step of the cases.
"""
import numpy as np

import inverse_dynamics_ref as idref

DOF = 6
FEASIBLE, EMPTY, STUCK, NONFINITE = 0, 1, 2, 3


def differences(P):
    """d, e [n, C, 6] of the points P [n, C, 6], in P's dtype: one operation each, as the law states them"""
    T = P.dtype.type
    d, e = np.zeros_like(P), np.zeros_like(P)
    d[:, 0] = P[:, 1] - P[:, 0]
    d[:, -1] = P[:, -1] - P[:, -2]
    d[:, 1:-1] = (P[:, 2:] - P[:, :-2]) * T(0.5)
    e[:, 1:-1] = (P[:, 2:] - T(2) * P[:, 1:-1]) + P[:, :-2]
    return d, e


def torque_rows(P, scales, gravity):
    """A, B, c [n, C, 6] in P's dtype: ID(p, 0, d), ID(p, d, e) without gravity, ID(p, 0, 0) with it"""
    n, C, _ = P.shape
    dt = P.dtype
    d, e = differences(P)
    flat = lambda x: np.ascontiguousarray(x).reshape(n * C, DOF)  # noqa: E731
    s = np.repeat(np.asarray(scales, dtype=dt), C, axis=0)
    zero = np.zeros((n * C, DOF), dtype=dt)
    with np.errstate(all="ignore"):
        A = idref.newton_euler(flat(P), zero, flat(d), s, 0.0, dt)
        B = idref.newton_euler(flat(P), flat(d), flat(e), s, 0.0, dt)
        c = idref.newton_euler(flat(P), zero, zero, s, gravity, dt)
    return tuple(x.reshape(n, C, DOF) for x in (A, B, c))


def velocity_bound(dk, v_max):
    """X [n] at one grid point: min over the moving joints of (v_max / |d|)^2; 0 where no joint moves"""
    T = dk.dtype.type
    a = np.abs(dk)
    with np.errstate(all="ignore"):
        r = np.asarray(v_max, dtype=dk.dtype) / a
        r2 = np.where(a > 0, r * r, T(np.inf))
    X = r2.min(axis=1)
    return np.where((a > 0).any(axis=1), X, T(0)).astype(dk.dtype)


def turned(A, B, c):
    """the rows with their sign turned so that A >= 0"""
    neg = A < 0
    return np.where(neg, -A, A), np.where(neg, -B, B), np.where(neg, -c, c)


def backward_step(A, B, c, lim, X, Knext):
    """One backward step by the pair rule, for n envs at once.  A, B, c, lim: [n, R] (sign not yet turned); X, Knext [n].
    Returns K [n], lo [n] (the largest lower bound, or 0), empty [n] (a zero slope with a negative right side)."""
    T = A.dtype.type
    n, R = A.shape
    a, b, cc = turned(A, B, c)
    la = np.concatenate([a, np.full((n, 1), T(2))], axis=1)
    lb = np.concatenate([b, np.full((n, 1), T(1))], axis=1)
    lL = np.concatenate([-lim - cc, np.zeros((n, 1), dtype=A.dtype)], axis=1)
    lH = np.concatenate([lim - cc, Knext[:, None].astype(A.dtype)], axis=1)
    with np.errstate(all="ignore"):
        slope = la[:, :, None] * lb[:, None, :] - la[:, None, :] * lb[:, :, None]        # [n, lower i, upper j]
        rhs = la[:, :, None] * lH[:, None, :] - la[:, None, :] * lL[:, :, None]
        bound = rhs / slope
    off = ~np.eye(R + 1, dtype=bool)[None]
    up = np.where((slope > 0) & off, bound, T(np.inf))
    dn = np.where((slope < 0) & off, bound, T(-np.inf))
    K = np.minimum(up.min(axis=(1, 2)), X)
    lo = np.maximum(dn.max(axis=(1, 2)), T(0))
    empty = ((slope == 0) & (rhs < 0) & off).any(axis=(1, 2))
    return K.astype(A.dtype), lo.astype(A.dtype), empty


def brute_backward_step(A, B, c, lim, X, Knext, tol=1e-9):
    """(min x, max x) over the polygon of one env's step, by enumerating vertices (float64); None when the polygon is empty.
    A, B, c, lim [R]; X, Knext scalars.  Half-planes g . (x, u) <= h."""
    G, H = [], []
    for Ai, Bi, ci, li in zip(A, B, c, lim):
        G += [(Bi, Ai), (-Bi, -Ai)]
        H += [li - ci, li + ci]
    G += [(-1.0, 0.0), (1.0, 0.0), (-1.0, -2.0), (1.0, 2.0)]
    H += [0.0, X, 0.0, Knext]
    G, H = np.array(G, dtype=np.float64), np.array(H, dtype=np.float64)
    scale = np.maximum(np.abs(G).max(axis=1), 1e-300)
    best = None
    m = len(G)
    for i in range(m):
        for j in range(i + 1, m):
            M = np.array([G[i], G[j]])
            det = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
            if abs(det) <= 1e-14 * scale[i] * scale[j]:
                continue
            v = np.array([H[i] * M[1, 1] - H[j] * M[0, 1], H[j] * M[0, 0] - H[i] * M[1, 0]]) / det
            if np.all(G @ v <= H + tol * (scale * (1.0 + np.abs(v).max()) + np.abs(H))):
                best = (v[0], v[0]) if best is None else (min(best[0], v[0]), max(best[1], v[0]))
    return best


def retime(P, v_max, a_max, tau_max=None, scales=None, gravity=0.0, dtype=np.float64, rows=None):
    """The whole law on points P [n, C, 6] (or [C, 6]).  tau_max None: no torque rows; else `scales` [n, 11] and `gravity`, or
    ready-made rows = (A, B, c) [n, C, 6] (e.g. the kernel's own workspace).  Returns a dict: feasible, duration, fail_at, reason,
    max_sdot, utilisation [n]; times, sdot2, K [n, C]; rows (A, B, c, lim) [n, C, R] with the sign as computed."""
    P = np.asarray(P, dtype=dtype)
    if P.ndim == 2:
        P = P[None]
    n, C, _ = P.shape
    T = P.dtype.type
    d, e = differences(P)
    A, B, c = d, e, np.zeros_like(d)
    lim = np.broadcast_to(np.asarray(a_max, dtype=dtype), (n, C, DOF))
    if tau_max is not None:
        tA, tB, tc = (np.asarray(x, dtype=dtype) for x in rows) if rows is not None else torque_rows(P, scales, gravity)
        A, B, c = (np.concatenate(p, axis=2) for p in ((A, tA), (B, tB), (c, tc)))
        lim = np.concatenate([lim, np.broadcast_to(np.asarray(tau_max, dtype=dtype), (n, C, DOF))], axis=2)
    lim = np.ascontiguousarray(lim)
    X = np.stack([velocity_bound(d[:, k], v_max) for k in range(C)], axis=1)
    finite_rows = np.isfinite(A).all(axis=2) & np.isfinite(B).all(axis=2) & np.isfinite(c).all(axis=2) & np.isfinite(d).all(axis=2) \
        & np.isfinite(e).all(axis=2)

    K = np.zeros((n, C), dtype=dtype)
    fail_at = np.full(n, -1)
    reason = np.zeros(n, dtype=int)
    for k in range(C - 2, -1, -1):
        Kk, lo, empty = backward_step(A[:, k], B[:, k], c[:, k], lim[:, k], X[:, k], K[:, k + 1])
        finite = finite_rows[:, k] & np.isfinite(Kk)
        with np.errstate(invalid="ignore"):
            empty = empty | (lo > Kk) | ((lo > 0) if k == 0 else False)
        bad = (fail_at < 0) & (~finite | empty)
        fail_at[bad] = k
        reason[bad] = np.where(finite[bad], EMPTY, NONFINITE)
        K[:, k] = np.where(finite, Kk, T(0))

    run = fail_at < 0
    x = np.zeros((n, C), dtype=dtype)
    times = np.zeros((n, C), dtype=dtype)
    util = np.zeros(n, dtype=dtype)
    stuck_at = np.full(n, -1)
    for k in range(C - 1):
        a, b, cc = turned(A[:, k], B[:, k], c[:, k])
        with np.errstate(all="ignore"):
            ui = ((lim[:, k] - cc) - b * x[:, k, None]) / a
            u = np.where(a > 0, ui, T(np.inf)).min(axis=1)
            x1 = np.minimum(np.maximum(x[:, k] + T(2) * u, T(0)), K[:, k + 1])
            uk = (x1 - x[:, k]) * T(0.5)
            util = np.maximum(util, (np.abs((a * uk[:, None] + b * x[:, k, None]) + cc) / lim[:, k]).max(axis=1))
            den = np.sqrt(x[:, k]) + np.sqrt(x1)
            stuck = run & (stuck_at < 0) & ~(den > 0)
            stuck_at[stuck] = k
            times[:, k + 1] = np.where(stuck_at < 0, times[:, k] + T(2) / den, T(np.inf))
        x[:, k + 1] = x1
    fail_at = np.where(run, stuck_at, fail_at)
    reason = np.where(run & (stuck_at >= 0), STUCK, reason)
    feasible = fail_at < 0
    times[~run, 1:] = np.inf
    x[~run] = 0
    return dict(feasible=feasible, duration=np.where(feasible, times[:, -1], T(np.inf)).astype(dtype), fail_at=fail_at, reason=reason,
                max_sdot=np.where(run, np.sqrt(x.max(axis=1)), T(0)).astype(dtype), utilisation=np.where(run, util, T(0)).astype(dtype),
                times=times, sdot2=x, K=K, rows=(A, B, c, lim), X=X)


def row_utilisation(P, sdot2, v_max, a_max, tau_max=None, scales=None, gravity=0.0, rows=None):
    """From a profile sdot2 [n, C] alone, in float64: (the largest |A u + B x + c| / LIM over every row of every interval [n],
    the largest x_k / X_k [n]) — what a feasible profile keeps <= 1."""
    P = np.asarray(P, dtype=np.float64)
    if P.ndim == 2:
        P = P[None]
    x = np.asarray(sdot2, dtype=np.float64)
    n, C, _ = P.shape
    d, e = differences(P)
    A, B, c = d, e, np.zeros_like(d)
    lim = np.broadcast_to(np.asarray(a_max, dtype=np.float64), (n, C, DOF))
    if tau_max is not None:
        tA, tB, tc = (np.asarray(r, dtype=np.float64) for r in rows) if rows is not None else torque_rows(P, scales, gravity)
        A, B, c = (np.concatenate(p, axis=2) for p in ((A, tA), (B, tB), (c, tc)))
        lim = np.concatenate([lim, np.broadcast_to(np.asarray(tau_max, dtype=np.float64), (n, C, DOF))], axis=2)
    u = (x[:, 1:] - x[:, :-1]) * 0.5
    val = np.abs(A[:, :-1] * u[:, :, None] + B[:, :-1] * x[:, :-1, None] + c[:, :-1]) / lim[:, :-1]
    X = np.stack([velocity_bound(d[:, k], v_max) for k in range(C)], axis=1)
    with np.errstate(all="ignore"):
        vel = np.where(x > 0, x / X, 0.0)
    return val.max(axis=(1, 2)), vel.max(axis=1)


def sample(P, times, sdot2, feasible, duration, t0, dt, T, dtype=np.float64, tau_dtype=None):
    """targets [n, T, 12] in `dtype` from a timed path: the law of pnr_sample_trajectory.  tau = t0 + (i + 1) dt is formed in
    `tau_dtype` (default `dtype`; product, then sum): with float32 the float64 evaluation looks at exactly the kernel's sample
    times and so at its intervals (qd jumps from one interval to the next: p_(k+1) - p_k changes)."""
    P = np.asarray(P, dtype=dtype)
    if P.ndim == 2:
        P = np.broadcast_to(P[None], (len(times),) + P.shape)
    times, x = np.asarray(times, dtype=dtype), np.asarray(sdot2, dtype=dtype)
    duration = np.asarray(duration, dtype=dtype)
    n, C, _ = P.shape
    F = P.dtype.type
    G = np.dtype(tau_dtype or dtype).type
    tau = (G(t0) + np.arange(1, T + 1).astype(G) * G(dt)).astype(dtype)        # [T]
    out = np.zeros((n, T, 2 * DOF), dtype=dtype)
    for env in range(n):
        if not feasible[env]:
            out[env, :, :DOF] = P[env, 0]
            continue
        past = ~(tau < duration[env])
        k = np.clip(np.searchsorted(times[env], tau, side="right") - 1, 0, C - 2)
        x0, x1 = x[env, k], x[env, k + 1]
        u = (x1 - x0) * F(0.5)
        v0 = np.sqrt(x0)
        dl = tau - times[env, k]
        sg = np.clip(v0 * dl + (u * (dl * dl)) * F(0.5), F(0), F(1))
        sd = v0 + u * dl
        dq = P[env, k + 1] - P[env, k]
        q = P[env, k] + sg[:, None] * dq
        qd = dq * sd[:, None]
        out[env, :, :DOF] = np.where(past[:, None], P[env, -1], q)
        out[env, :, DOF:] = np.where(past[:, None], F(0), qd)
    return out
