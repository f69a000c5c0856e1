"""Independent reference of pnr_path_clearance, float64 (and float32), built on contact_query_ref.query's `dist` (every sample's
distance to every body); it imports nothing of pioneer_amd.  The law it restates (include/pioneer_amd.h):

* THE PATH: W waypoints, M sub-steps per segment, C = 1 + (W - 1) M configurations.  Configuration 0 is waypoint 0; configuration
  1 + i M + (j - 1), j = 1 .. M, lies on segment i from a = waypoint i to b = waypoint i + 1: a + (j / M)(b - a), evaluated in
  the arithmetic's dtype, for j < M and EXACTLY b for j = M.  Its path coordinate is t = i + j / M (0 for configuration 0).
* THE -inf RULE: a (sample, body) distance that is not finite counts as -inf, so the order is total and a NaN waypoint makes the
  path not free.  Without bodies a configuration's clearance is +inf.
* THE TIE RULES: a configuration's clearance is the smallest distance over the samples of the mask and the bodies; within it the
  lowest sample wins, then the lowest body; over the path the lowest configuration wins.
* THE SUMMARY: the smallest clearance, its t, its sample and body (0 and -1 without bodies), t of the first configuration with
  clearance < margin (-1: none), the number of such configurations, 1 if there is none else 0, 0.
"""
import numpy as np

import contact_query_ref as cq

SUMMARY_DIM = 8
ALL_SAMPLES = (1 << cq.SAMPLES) - 1


def path_coordinates(W, M, dtype=np.float64):
    """t [C] as the law states it; in float32 the division and the sum are float32's"""
    dtype = np.dtype(dtype).type
    t = np.zeros(1 + (W - 1) * M, dtype=dtype)
    for i in range(W - 1):
        for j in range(1, M + 1):
            t[1 + i * M + (j - 1)] = dtype(i + 1) if j == M else dtype(i) + dtype(j) / dtype(M)
    return t


def configurations(waypoints, M, dtype=np.float64):
    """q [N, C, 6] of the waypoints [N, W, 6]"""
    dtype = np.dtype(dtype).type
    w = np.asarray(waypoints).astype(dtype)
    N, W, _ = w.shape
    q = np.empty((N, 1 + (W - 1) * M, 6), dtype=dtype)
    q[:, 0] = w[:, 0]
    for i in range(W - 1):
        a, b = w[:, i], w[:, i + 1]
        for j in range(1, M + 1):
            q[:, 1 + i * M + (j - 1)] = b if j == M else a + (dtype(j) / dtype(M)) * (b - a)
    return q


def sweep(waypoints, M, bodies, body_positions=None, margin=0.0, mask=ALL_SAMPLES, pointer_radius=0.2, dtype=np.float64):
    """dict: clearance [N, C] (the profile), pairs [N, C, 23, nb] (every (sample, body) distance after the -inf rule, +inf for a
    sample outside the mask), t [C], q [N, C, 6], summary [N, 8], config [N] (the configuration of the minimum),
    first [N] (the first violating configuration, -1: none)."""
    q = configurations(waypoints, M, dtype)
    N, C, _ = q.shape
    nb = len(bodies)
    t = path_coordinates(np.asarray(waypoints).shape[1], M)
    if nb:
        bp = None if body_positions is None else np.repeat(np.asarray(body_positions).reshape(N, nb, 3), C, axis=0)
        flat = q.reshape(N * C, 6)
        with np.errstate(invalid="ignore"):
            d = cq.query(flat, np.zeros_like(flat), bodies, bp, pointer_radius=pointer_radius, dtype=dtype)["dist"].astype(np.float64)
        d = np.where(np.isfinite(d), d, -np.inf).reshape(N, C, cq.SAMPLES, nb)
    else:
        d = np.full((N, C, cq.SAMPLES, 1), np.inf)
    off = np.array([not (mask >> s) & 1 for s in range(cq.SAMPLES)])
    d[:, :, off, :] = np.inf
    flat = d.reshape(N, C, -1)
    k = np.argmin(flat, axis=2)                          # the first of equal values: the lowest sample, then the lowest body
    clearance = np.take_along_axis(flat, k[:, :, None], axis=2)[:, :, 0]
    sample, body = k // d.shape[3], k % d.shape[3]
    none = np.isposinf(clearance)                        # no (sample, body) pair at all
    sample, body = np.where(none, 0, sample), np.where(none, -1, body)
    c = np.argmin(clearance, axis=1)                     # .. the lowest configuration
    rows = np.arange(N)
    hit = clearance < margin
    first = np.where(hit.any(axis=1), np.argmax(hit, axis=1), -1)
    summary = np.zeros((N, SUMMARY_DIM))
    summary[:, 0], summary[:, 1], summary[:, 2], summary[:, 3] = clearance[rows, c], t[c], sample[rows, c], body[rows, c]
    summary[:, 4] = np.where(first >= 0, t[np.maximum(first, 0)], -1.0)
    summary[:, 5], summary[:, 6] = hit.sum(axis=1), ~hit.any(axis=1)
    return dict(clearance=clearance, pairs=d, t=t, q=q, summary=summary, config=c, first=first)


def near_margin(clearance, margin, within=1e-3):
    """[N, C] bool: the configurations whose clearance a float32 evaluation may put on the other side of the margin"""
    return np.abs(clearance - margin) < within
