"""Independent reference of pnr_get_contacts: the arm's 23 contact sample spheres against static planes, boxes and spheres.

Built from tests/golden/urdf_chain.json (through link_kinematics_ref.link_frames) and its own copy of the sample table; it
imports nothing of pioneer_amd.  `body_distance` is the one statement under tests/ of the plane / sphere / box signed distance
(tests/moving_sphere_ref.py takes its static world from it).  The law it restates (include/pioneer_amd.h):

* sample s is a sphere (centre c_s in the frame of URDF link L_s, radius r_s; the needle's three samples take the pointer's
  radius) and touches every body with its surface: distance = sdf_body(centre) - r_s;
* plane: n . (x - o) with n the body's rotated unit normal; sphere: |x - o| - R, normal (x - o) / |x - o|; oriented box: the
  usual exterior distance, and inside, out through the nearest face (the largest of |l_k| - h_k);
* force of body b on sample s: f = max(0, kp depth - kd (v . n)) if depth = -distance > 0 else 0, along n;
* record of sample s: the nearest body's (distance, n, centre - r n, b, f); summary: the smallest distance, its sample, its body,
  the number of samples with distance < 0; tau_j = sum_s a_j . ((x_s - o_j) x F_s), F_s the sum over all bodies.

`query(..., dtype=np.float32)` runs the same arithmetic in float32 (link_frames in float32, the joints' rotations written entry
by entry: link_kinematics_ref.coordinate_rotation): the difference to float64 on the same inputs is what float32 alone costs,
whatever the order of operations.
"""
import numpy as np

import link_kinematics_ref as lk

SAMPLES = 23
DIM = 9
# (URDF link index, a, b, n, radius): n spheres from a to b in the link's frame; radius < 0 = the pointer's radius.  The last
# sample of the last capsule is the pointer's own sphere (robot:pointer sits at (3.6, 0, 1.9) in the effector's frame).
CAPSULES = (
    (3, (0.0, 0.0, 0.0), (0.0, 0.0, 11.0), 8, 0.7),        # arm1
    (4, (-1.0, 1.0, 0.0), (9.0, 1.0, 0.0), 7, 0.7),        # arm2
    (5, (9.0, 0.0, 0.0), (11.0, 0.0, 0.0), 2, 0.7),        # rotator2 + hinge2
    (7, (-0.5, 0.0, 0.0), (2.5, 0.0, 0.0), 3, 0.6),        # arm3
    (9, (3.6, 0.0, -0.75), (3.6, 0.0, 1.9), 3, -1.0),      # the effector's needle
)
LINK_TO_BODY = {3: 1, 4: 2, 5: 3, 7: 4, 9: 5}               # the engine's merged moving body (0-based) that carries the link
# the link PyBullet would report for a sample (linkIndexA): the capsule's link; the pointer's sphere is link 10
SAMPLE_LINKS = (3,) * 8 + (4,) * 7 + (5,) * 2 + (7,) * 3 + (9,) * 2 + (10,)
# arm2's last sample, (9, 1, 0) in arm2, and rotator2's first, (9, 0, 0) in rotator2 (whose origin is (0, 1, 0) in arm2), are the
# same sphere: their distances tie to rounding, so a comparison of the summary's sample index counts them as one
TWIN_SAMPLES = (14, 15)


def merge_twins(sample_index):
    idx = np.asarray(sample_index)
    return np.where(idx == TWIN_SAMPLES[1], TWIN_SAMPLES[0], idx)


# child link of revolute joint j
JOINT_LINKS = (1, 3, 4, 5, 7, 8)


def sample_table():
    """[(link, centre[3], radius)] x 23, in table order"""
    out = []
    for link, a, b, n, radius in CAPSULES:
        a, b = np.asarray(a), np.asarray(b)
        for i in range(n):
            t = i / (n - 1) if n > 1 else 0.0
            out.append((link, a + t * (b - a), radius))
    assert len(out) == SAMPLES
    return out


def plane(normal, position=(0.0, 0.0, 0.0), quat=(0.0, 0.0, 0.0, 1.0)):
    return dict(shape="plane", position=tuple(map(float, position)), quat=tuple(map(float, quat)), size=tuple(map(float, normal)))


def box(half_extents, position, quat=(0.0, 0.0, 0.0, 1.0)):
    return dict(shape="box", position=tuple(map(float, position)), quat=tuple(map(float, quat)), size=tuple(map(float, half_extents)))


def sphere(radius, position):
    return dict(shape="sphere", position=tuple(map(float, position)), quat=(0.0, 0.0, 0.0, 1.0), size=(float(radius), 0.0, 0.0))


def body_frame(b):
    """float64: the body's rotation from its quaternion (x, y, z, w), normalised; a plane's unit world normal"""
    R = lk.matrix_from_quat(b["quat"])
    normal = None
    if b["shape"] == "plane":
        nrm = np.asarray(b["size"], dtype=np.float64)
        normal = R @ nrm / np.linalg.norm(nrm)
    return R, normal


def body_distance(b, o, x, dtype):
    """sdf [N] and unit normal [N, 3] of the points x [N, 3] against body b placed at o [N, 3] (or [3]); also `gap` [N]: inside
    a box, the difference between the two largest of |l_k| - h_k (the nearest-face switch); +inf elsewhere"""
    R64, normal = body_frame(b)
    dd = x - np.asarray(o, dtype=dtype)
    gap = np.full(x.shape[0], np.inf)
    if b["shape"] == "plane":
        nrm = np.broadcast_to(normal.astype(dtype), x.shape)
        return dd @ normal.astype(dtype), nrm, gap
    if b["shape"] == "sphere":
        ln = np.sqrt((dd * dd).sum(axis=1))
        safe = np.where(ln > 0, ln, dtype(1))
        nrm = np.where((ln > 0)[:, None], dd / safe[:, None], np.asarray([0, 0, 1], dtype=dtype))
        return ln - dtype(b["size"][0]), nrm, gap
    R = R64.astype(dtype)
    h = np.asarray(b["size"], dtype=dtype)
    l = dd @ R                                             # R^T dd
    qq = np.abs(l) - h
    o_ = np.maximum(qq, dtype(0))
    out2 = (o_ * o_).sum(axis=1)
    outside = out2 > 0
    ln = np.sqrt(np.where(outside, out2, dtype(1)))
    sg = np.where(l < 0, dtype(-1), dtype(1))
    n_out = sg * o_ / ln[:, None]
    km = np.where((qq[:, 0] >= qq[:, 1]) & (qq[:, 0] >= qq[:, 2]), 0, np.where(qq[:, 1] >= qq[:, 2], 1, 2))
    n_in = np.zeros_like(l)
    n_in[np.arange(l.shape[0]), km] = sg[np.arange(l.shape[0]), km]
    sdf = np.where(outside, ln, qq[np.arange(l.shape[0]), km])
    nl = np.where(outside[:, None], n_out, n_in)
    srt = np.sort(qq.astype(np.float64), axis=1)
    gap = np.where(outside, np.inf, srt[:, 2] - srt[:, 1])
    return sdf, nl @ R.T, gap


def query(q, qd, bodies, body_positions=None, kp=2000.0, kd=50.0, pointer_radius=0.2, dtype=np.float64):
    """The three outputs of pnr_get_contacts and what the comparisons' exclusions need, all [N, ...]:
    points [N, 23, 9], summary [N, 4], torques [N, 6]; centres, velocities [N, 23, 3]; dist [N, 23, nb] (every body's distance);
    force [N, 23, 3] (F_s over all bodies); box_gap [N, 23] (the smallest nearest-face gap over the boxes the centre is inside);
    lever [N] (the longest |x_s - o_j| over the samples and their inboard joints)."""
    dtype = np.dtype(dtype).type
    R, p, v, w = lk.link_frames(q, qd, dtype=dtype, rotation=lk.axis_rotation if dtype is np.float64 else lk.coordinate_rotation)
    n, nb = p.shape[0], len(bodies)
    kp, kd = dtype(kp), dtype(kd)
    bp = None if body_positions is None else np.asarray(body_positions, dtype=dtype).reshape(n, nb, 3)
    points = np.zeros((n, SAMPLES, DIM), dtype=dtype)
    centres = np.zeros((n, SAMPLES, 3), dtype=dtype); vels = np.zeros_like(centres); force = np.zeros_like(centres)
    dist = np.zeros((n, SAMPLES, nb), dtype=dtype)
    box_gap = np.full((n, SAMPLES), np.inf)
    torques = np.zeros((n, 6), dtype=dtype)
    lever = np.zeros(n)
    for s, (link, c, radius) in enumerate(sample_table()):
        r = dtype(pointer_radius if radius < 0 else radius)
        rel = R[:, link] @ c.astype(dtype)
        x = p[:, link] + rel
        vel = v[:, link] + np.cross(w[:, link], rel)
        centres[:, s], vels[:, s] = x, vel
        best = np.full(n, np.inf, dtype=dtype); bestn = np.zeros((n, 3), dtype=dtype)
        bestb = np.full(n, -1, dtype=dtype); bestf = np.zeros(n, dtype=dtype)
        F = np.zeros((n, 3), dtype=dtype)
        for b, body in enumerate(bodies):
            o = bp[:, b] if bp is not None else np.asarray(body["position"], dtype=dtype)
            sdf, nrm, gap = body_distance(body, o, x, dtype)
            d = sdf - r
            depth = -d
            fn = kp * depth - kd * (vel * nrm).sum(axis=1)
            f = np.where((depth > 0) & (fn > 0), fn, dtype(0))
            F = F + f[:, None] * nrm
            dist[:, s, b] = d
            box_gap[:, s] = np.minimum(box_gap[:, s], gap)
            take = d < best
            best = np.where(take, d, best); bestn = np.where(take[:, None], nrm, bestn)
            bestb = np.where(take, dtype(b), bestb); bestf = np.where(take, f, bestf)
        points[:, s, 0] = best; points[:, s, 1:4] = bestn; points[:, s, 4:7] = x - r * bestn
        points[:, s, 7] = bestb; points[:, s, 8] = bestf
        force[:, s] = F
        for j, jl in enumerate(JOINT_LINKS):
            if jl > link:
                continue
            axis = R[:, jl][:, :, [2, 1, 1, 0, 1, 0][j]]
            arm = x - p[:, jl]
            torques[:, j] += (axis * np.cross(arm, F)).sum(axis=1)
            lever = np.maximum(lever, np.linalg.norm(arm.astype(np.float64), axis=1))
    d0 = points[:, :, 0]
    k = np.argmin(d0, axis=1)
    rows = np.arange(n)
    summary = np.stack([d0[rows, k], k.astype(dtype), points[rows, k, 7], (d0 < 0).sum(axis=1).astype(dtype)], axis=1).astype(dtype)
    return dict(points=points, summary=summary, torques=torques, centres=centres, velocities=vels, dist=dist, force=force,
                box_gap=box_gap, lever=lever)


def exclusions(ref, tie=1e-3, zero=1e-3):
    """What a comparison may leave out, from the float64 reference alone, per (env, sample):
    geometry: the two nearest bodies within `tie`, or inside a box with its two largest interior coordinates within `tie`;
    force: geometry, or any body's |distance| < `zero` (the kd term switches on there)."""
    dist = ref["dist"].astype(np.float64)
    n, S, nb = dist.shape
    near_tie = np.zeros((n, S), dtype=bool)
    if nb >= 2:
        srt = np.sort(dist, axis=2)
        near_tie = (srt[:, :, 1] - srt[:, :, 0]) < tie
    geometry = near_tie | (ref["box_gap"] < tie)
    near_zero = (np.abs(dist) < zero).any(axis=2) if nb else np.zeros((n, S), dtype=bool)
    return dict(geometry=geometry, force=geometry | near_zero)
