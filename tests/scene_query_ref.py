"""The float64 references of the scene queries' per-env world, composed per env from the existing references, which are not
edited: render_ref.render_pixels and ray_ref.trace / resolve see env k's bodies at env k's positions with the moving sphere
appended as one more static sphere (the last body, so it loses a tie to the caller's bodies) and its label rewritten to 21;
contact_query_ref.query gives the caller's bodies, and the moving sphere's law is stated here (include/pioneer_amd.h,
pnr_get_contacts):

    distance = |p_s - x| - radius - r_s;  n = (p_s - x) / |p_s - x|, (0, 0, -1) at zero distance;
    force = max(0, kp depth - kd ((v_s - v) . n)) where depth = -distance > 0, along n on the sample;

the sphere is body 8; it is a sample's nearest body where its distance is STRICTLY smaller than every caller's body's; F_s and the
joint torques include its force.  An env whose mass word is <= 0 has no sphere.  Imports nothing of pioneer_amd.
"""
import numpy as np

import contact_query_ref as cq
import link_kinematics_ref as lk
import ray_ref as ry
import render_ref as rr

SEG_MOVING_BODY = 21
BODY_MOVING = 8
SPHERE_RGBA = (0.3, 0.3, 0.3, 1.0)            # the URDF's obstacle_mat: the colour a handle draws its sphere in until told another


def env_bodies(bodies, positions, words, rgba=SPHERE_RGBA):
    """(shape, position, orientation, size, rgba) per body of one env: the caller's (SceneBody, rgba) pairs at `positions` [nb, 3]
    (None: their own), then the moving sphere of the env's words [8] if its mass is > 0; and the appended body's label, or None"""
    out = [(b.shape, b.position if positions is None else tuple(map(float, positions[i])), b.orientation, b.size, col)
           for i, (b, col) in enumerate(bodies)]
    if words is None or not float(words[6]) > 0.0:
        return out, None
    out.append(("sphere", tuple(map(float, words[0:3])), (0.0, 0.0, 0.0, 1.0), (float(words[7]), 0.0, 0.0), rgba))
    return out, rr.SEG_BODY0 + len(out) - 1


def _relabel(labels, appended):
    labels = np.asarray(labels).copy()
    if appended is not None:
        labels[labels == appended] = SEG_MOVING_BODY
    return labels


def render_env(q, target, cfg, view, bodies, positions=None, words=None, rgba=SPHERE_RGBA):
    """render_ref.render_pixels at every pixel of one env's image (cfg: width, height, fov, near, far)"""
    W, H = cfg.render_width, cfg.render_height
    yy, xx = np.mgrid[0:H, 0:W]
    eb, appended = env_bodies(bodies, positions, words, rgba)
    want = rr.render_pixels(np.asarray(q, dtype=np.float64), np.asarray(target, dtype=np.float64), xx.ravel(), yy.ravel(), view,
                            cfg.projection_fov, cfg.projection_near, cfg.projection_far, W, H, bodies=eb)
    want["seg"] = _relabel(want["seg"], appended).astype(np.uint8)
    want["behind"] = _relabel(want["behind"], appended).astype(np.uint8)
    return want


def rays_env(q, target, rays, mask, bodies, positions=None, words=None, parent_link=-1):
    """ray_ref's answers for one env's rays [R, 6]; also the trace (for the rays' world lengths)"""
    eb, appended = env_bodies(bodies, positions, words)
    tr = ry.trace(np.asarray(q, dtype=np.float64), np.asarray(target, dtype=np.float64), rays, eb, parent_link)
    want = ry.resolve(tr, mask)
    want["label"] = _relabel(want["label"], appended)
    return want, tr


def contacts(q, qd, bodies, body_positions, words, kp=2000.0, kd=50.0, pointer_radius=0.2):
    """pnr_get_contacts' three outputs [N, ...] with the moving spheres of words [N, 8] (None: no sphere anywhere), and what
    contact_query_ref.exclusions needs: `dist` has one more column, the sphere's distance (+inf where an env has none).
    bodies: contact_query_ref's body dicts."""
    base = cq.query(q, qd, bodies, body_positions, kp, kd, pointer_radius)
    if words is None:
        return base
    n = base["points"].shape[0]
    w = np.asarray(words, dtype=np.float64)
    x, v, there, radius = w[:, None, 0:3], w[:, None, 3:6], w[:, 6] > 0.0, w[:, 7:8]
    sample_r = np.array([pointer_radius if r < 0 else r for _, _, r in cq.sample_table()])[None, :]
    dd = base["centres"] - x                                         # [N, 23, 3]
    ln = np.linalg.norm(dd, axis=2)
    nrm = np.where((ln > 0)[..., None], dd / np.where(ln > 0, ln, 1.0)[..., None], np.array([0.0, 0.0, -1.0]))
    dist = np.where(there[:, None], ln - radius - sample_r, np.inf)
    depth = -dist
    fn = kp * depth - kd * ((base["velocities"] - v) * nrm).sum(axis=2)
    f = np.where((depth > 0) & (fn > 0), fn, 0.0)                    # (no sphere: depth = -inf)
    pts = base["points"].copy()
    take = dist < pts[:, :, 0]
    pts[:, :, 0] = np.where(take, dist, pts[:, :, 0])
    pts[:, :, 1:4] = np.where(take[..., None], nrm, pts[:, :, 1:4])
    pts[:, :, 4:7] = np.where(take[..., None], base["centres"] - sample_r[..., None] * nrm, pts[:, :, 4:7])
    pts[:, :, 7] = np.where(take, float(BODY_MOVING), pts[:, :, 7])
    pts[:, :, 8] = np.where(take, f, pts[:, :, 8])
    Fs = f[..., None] * nrm                                          # the sphere's force on every sample
    R, p, _, _ = lk.link_frames(np.asarray(q, dtype=np.float64), np.asarray(qd, dtype=np.float64))
    tau = base["torques"].copy()
    for s, (link, _, _) in enumerate(cq.sample_table()):
        for j, jl in enumerate(cq.JOINT_LINKS):
            if jl <= link:
                axis = R[:, jl][:, :, [2, 1, 1, 0, 1, 0][j]]
                tau[:, j] += (axis * np.cross(base["centres"][:, s] - p[:, jl], Fs[:, s])).sum(axis=1)
    d0 = pts[:, :, 0]
    k = np.argmin(d0, axis=1)
    rows = np.arange(n)
    summary = np.stack([d0[rows, k], k.astype(np.float64), pts[rows, k, 7], (d0 < 0).sum(axis=1).astype(np.float64)], axis=1)
    return dict(base, points=pts, summary=summary, torques=tau, force=base["force"] + Fs,
                dist=np.concatenate([base["dist"], dist[..., None]], axis=2), sphere_force=f, sphere_dist=dist)
