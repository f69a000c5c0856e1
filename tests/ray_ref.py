"""Independent float64 reference of pnr_ray_test: segments against the URDF's visual shapes, the target and static bodies.

Built from render_ref.scene_prims (tests/golden/urdf_visuals.json posed by link_kinematics_ref.link_frames), render_ref's
solid_interval (the line against a sphere, box or capped cylinder) and normal_at; it does not read the engine, its tables or
pioneer_amd.  Rules (include/pioneer_amd.h, pnr_ray_test): ray r is from + t (to - from), t in [0, 1]; every shape is a solid (a plane: the half-space below its surface); a ray hits a solid at
its entering parameter t_n if it starts outside it and 0 <= t_n <= 1; the smallest t_n wins, on a tie the order is arm visuals
(table order), the target, bodies by index; a zero-length ray misses.  With parent_link >= 0 the rays are given in that URDF
link's frame of the env.

The ambiguity band marks rays where either answer may be right: the label changes when `to` moves by 1e-4 of the ray's length
along any axis; the two nearest candidates of different labels lie within 1e-5 in t; a candidate's t_n lies within 1e-5 of 0 or
1; `from` lies within 1e-4 units of an enabled solid's surface ("starts inside" is undecidable); or the winning hit lies on an
edge of a box or cylinder (normal_at's edge flag).
"""
import numpy as np

import link_kinematics_ref as lk
import render_ref as rr

HIT_BODIES, HIT_ARM, HIT_TARGET = 1, 2, 4
GREY = (0.5, 0.5, 0.5, 1.0)


def solids(q, target, bodies=(), target_radius=0.2, data=None):
    """Every primitive of one env in tie order: arm visuals (table order), the target, bodies by index.
    bodies: (shape, position, orientation (x, y, z, w), size) per body (a fifth entry, a colour, is ignored)."""
    prims = rr.scene_prims(q, target, target_radius, bodies=[(b[0], b[1], b[2], b[3], GREY) for b in bodies], data=data)
    arm = [P for P in prims if rr.SEG_LINK0 <= P["label"] < rr.SEG_TARGET]
    tgt = [P for P in prims if P["label"] == rr.SEG_TARGET]
    bod = [P for P in prims if P["label"] >= rr.SEG_BODY0]
    return arm + tgt + bod


def enabled(prims, mask):
    """Which of `solids`' primitives the hit mask enables [P] bool."""
    lab = np.array([P["label"] for P in prims])
    return (((lab < rr.SEG_TARGET) & bool(mask & HIT_ARM)) | ((lab == rr.SEG_TARGET) & bool(mask & HIT_TARGET))
            | ((lab >= rr.SEG_BODY0) & bool(mask & HIT_BODIES)))


def intersect(P, O, D):
    """(tn, tf) of the lines O[m] + t D[m] against the solid P; tn > tf where the line misses it."""
    if P["kind"] != rr.PLANE:
        return rr.solid_interval(P, O, D)
    # pnr_ray_test's plane is the half-space n . (x - c) <= 0 below it (pnr_render's is the surface alone, render_ref.intersect):
    # { t : on + t dn <= 0 } is [t0, inf) going down, (-inf, t0] going up, all or nothing along the surface
    on, dn = (O - P["c"][None]) @ P["n"], D @ P["n"]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -on / dn
    tn = np.where(dn < 0, t, np.where((dn > 0) | (on <= 0), -np.inf, np.inf))
    tf = np.where(dn > 0, t, np.where((dn < 0) | (on <= 0), np.inf, -np.inf))
    return tn, tf


def surface_distance(P, X):
    """|signed distance| of the points X [M, 3] to the surface of the solid P."""
    if P["kind"] == rr.PLANE:
        return np.abs((X - P["c"][None]) @ P["n"])
    x = (X - P["c"][None]) @ P["R"]
    if P["kind"] == rr.SPHERE:
        return np.abs(np.linalg.norm(x, axis=1) - P["half"][0])
    if P["kind"] == rr.BOX:
        qd = np.abs(x) - P["half"][None]
    else:
        qd = np.stack([np.hypot(x[:, 0], x[:, 1]) - P["half"][0], np.abs(x[:, 2]) - P["half"][2]], axis=1)
    outside = np.linalg.norm(np.maximum(qd, 0), axis=1)
    return np.abs(outside + np.minimum(qd.max(axis=1), 0))


def _candidates(prims, O, D):
    """T [P, M]: each solid's counted entering parameter (inf where it is not hit); TN [P, M]: every line-solid entering parameter."""
    M = len(O)
    T, TN = np.full((len(prims), M), np.inf), np.full((len(prims), M), np.inf)
    nonzero = np.einsum("ij,ij->i", D, D) > 0
    for i, P in enumerate(prims):
        tn, tf = intersect(P, O, D)
        meets = (tn <= tf) & nonzero
        TN[i] = np.where(meets, tn, np.inf)
        T[i] = np.where(meets & (tn >= 0) & (tn <= 1), tn, np.inf)
    return T, TN


def _winner(lab, T):
    """(row, t, label) of the nearest counted candidate per ray; the first of equal minima: the tie order."""
    if not len(lab):
        return np.zeros(T.shape[1], int), np.full(T.shape[1], np.inf), np.zeros(T.shape[1], int)
    i = np.argmin(T, axis=0)
    t = T[i, np.arange(T.shape[1])]
    return i, t, np.where(np.isfinite(t), lab[i], 0)


def world_rays(q, rays, parent_link=-1):
    """rays [M, 6] of one env from the frame of URDF link parent_link (-1: already the world frame) to the world frame."""
    rays = np.asarray(rays, dtype=np.float64)
    if parent_link < 0:
        return rays[:, 0:3], rays[:, 3:6]
    R, p, _, _ = lk.link_frames(np.asarray(q, dtype=np.float64)[None])
    R, p = R[0, parent_link], p[0, parent_link]
    return p[None] + rays[:, 0:3] @ R.T, p[None] + rays[:, 3:6] @ R.T


def trace(q, target, rays, bodies=(), parent_link=-1, target_radius=0.2, data=None):
    """Everything about the rays [M, 6] of one env that does not depend on the hit mask: every solid's candidates for the rays
    and for `to` moved by +-1e-4 of the length along each axis, and the distance of `from` to every surface."""
    prims = solids(q, target, bodies, target_radius, data)
    O, E = world_rays(q, rays, parent_link)
    D = E - O
    M = len(O)
    length = np.linalg.norm(D, axis=1)
    moved = [D]
    for k in range(3):
        for s in (1.0, -1.0):
            D2 = D.copy()
            D2[:, k] += s * 1e-4 * length
            moved.append(D2)
    T, TN = _candidates(prims, np.tile(O, (7, 1)), np.concatenate(moved))
    T, TN = T.reshape(len(prims), 7, M), TN.reshape(len(prims), 7, M)
    near = np.array([surface_distance(P, O) <= 1e-4 for P in prims]).reshape(len(prims), M)
    return dict(prims=prims, O=O, E=E, D=D, T=T[:, 0], TN=TN[:, 0], T_moved=T[:, 1:], near=near)


def resolve(tr, mask):
    """One env's answers under a hit mask, from `trace`: fraction [M], position [M, 3], normal [M, 3], label [M], band [M]."""
    on = enabled(tr["prims"], mask)
    prims = [P for P, k in zip(tr["prims"], on) if k]
    lab = np.array([P["label"] for P in prims], dtype=np.int64)
    O, E, D, T, TN = tr["O"], tr["E"], tr["D"], tr["T"][on], tr["TN"][on]
    M = len(O)
    win, t, label = _winner(lab, T)
    hit = np.isfinite(t)
    fraction = np.where(hit, t, 1.0)
    position = np.where(hit[:, None], O + np.where(hit, t, 0.0)[:, None] * D, E)
    normal = np.zeros((M, 3))
    band = tr["near"][on].any(axis=0) if len(prims) else np.zeros(M, bool)      # "starts inside" is undecidable
    for i, P in enumerate(prims):
        sel = hit & (win == i)
        if sel.any():
            nrm, edge = rr.normal_at(P, np.zeros(3), position[sel], np.ones(int(sel.sum())))
            normal[sel] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
            band[sel] |= edge
    for k in range(6):                                                  # the label under a moved `to`
        band |= _winner(lab, tr["T_moved"][on][:, k])[2] != label
    if len(prims):
        with np.errstate(invalid="ignore"):                              # inf - inf where fewer than two candidates exist
            order = np.argsort(T, axis=0, kind="stable")
            Ts = np.take_along_axis(T, order, axis=0)
            for r in range(1, len(prims)):
                band |= (lab[order[r]] != lab[order[0]]) & np.isfinite(Ts[r]) & (Ts[r] - Ts[0] <= 1e-5)
            band |= (np.isfinite(TN) & ((np.abs(TN) <= 1e-5) | (np.abs(TN - 1.0) <= 1e-5))).any(axis=0)
    return dict(fraction=fraction, position=position, normal=normal, label=label.astype(np.int64), band=band)


def ray_test(q, target, rays, mask, bodies=(), parent_link=-1, target_radius=0.2, data=None):
    """resolve(trace(...), mask)."""
    return resolve(trace(q, target, rays, bodies, parent_link, target_radius, data), mask)
