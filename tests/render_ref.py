"""Independent float64 reference of pnr_render: camera images of the URDF's visual shapes, the target and static bodies.

Built from tests/golden/urdf_visuals.json (the URDF's visual numbers), link_kinematics_ref.link_frames (the URDF chain) and
the view matrix the caller passes in; it does not read the engine, its tables or pioneer_amd.  Rules (include/pioneer_amd.h,
pnr_render): pixel (x, y) is the ray through ndc (2(x + 0.5)/W - 1, 1 - 2(y + 0.5)/H) of a vertical-fov perspective with
aspect W/H; per primitive the entering and leaving intersections are candidates, counted when their eye depth lies in
(near, far); the nearest opaque candidate wins; the target sphere is translucent (alpha blend before quantisation, seg and depth
report it); c = clamp(rgb (ambient + diffuse max(0, n . l)), 0, 1) with n facing the viewer; byte = floor(255 c + 0.5).

Pixels may be given at any (fractional) coordinates.  The ambiguity band marks pixels where either label may be right: the
label (and under the target the label behind it) changes when the ray moves +-0.01 px in x or y; the two nearest candidates
of different labels lie within 1e-5 relative depth; a candidate lies within 1e-5 relative of near or far; or the winning hit
lies on an edge of its shape (within 1e-5), where the face normal, and so the colour, is undetermined.
"""
import json
import os

import numpy as np

import link_kinematics_ref as lk

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "urdf_visuals.json")
SEG_BACKGROUND, SEG_LINK0, SEG_TARGET, SEG_BODY0 = 0, 1, 12, 13
BOX, CYLINDER, SPHERE, PLANE = "box", "cylinder", "sphere", "plane"


def load_visuals(path=GOLDEN):
    with open(path) as f:
        return json.load(f)


def scene_prims(q, target, target_radius=0.2, target_rgba=(1.0, 0.0, 0.0, 0.5), bodies=(), data=None):
    """Primitives of one env: dicts with kind, R (shape frame -> world), c (centre), half, rgb, label, alpha (None = opaque).
    q: the env's 6 joints; bodies: (shape, position, orientation (x, y, z, w), size, rgba) per static body."""
    data = data or load_visuals()
    chain = lk.load_chain()
    links = [j["child"] for j in chain]
    R, p, _, _ = lk.link_frames(np.asarray(q, dtype=np.float64)[None], None, chain)
    prims = []
    for v in data["visuals"]:
        k = links.index(v["link"])
        Rv = lk.rpy_rotation([float(s) for s in v["rpy"]])
        Rw = R[0, k] @ Rv
        c = p[0, k] + R[0, k] @ np.asarray(v["xyz"], dtype=np.float64)
        g = v["geometry"]
        if g["type"] == BOX:
            half = 0.5 * np.asarray(g["size"], dtype=np.float64)
        elif g["type"] == CYLINDER:
            half = np.array([g["radius"], g["radius"], 0.5 * g["length"]])
        else:
            half = np.array([g["radius"]] * 3)
        rgba = data["materials"][v["material"]]
        prims.append(dict(kind=g["type"], R=Rw, c=c, half=half, rgb=np.asarray(rgba[:3], dtype=np.float64), label=SEG_LINK0 + k,
                          alpha=None))
    for b, (shape, pos, orn, size, rgba) in enumerate(bodies):
        Rb = lk.matrix_from_quat(orn)
        size = np.asarray(size, dtype=np.float64)
        if shape == PLANE:
            n = Rb @ size / np.linalg.norm(size)
            prims.append(dict(kind=PLANE, R=None, n=n, c=np.asarray(pos, dtype=np.float64), half=None,
                              rgb=np.asarray(rgba[:3], dtype=np.float64), label=SEG_BODY0 + b, alpha=None))
        else:
            half = size if shape == BOX else np.array([size[0]] * 3)
            prims.append(dict(kind=shape, R=Rb, c=np.asarray(pos, dtype=np.float64), half=half,
                              rgb=np.asarray(rgba[:3], dtype=np.float64), label=SEG_BODY0 + b, alpha=None))
    prims.append(dict(kind=SPHERE, R=np.eye(3), c=np.asarray(target, dtype=np.float64), half=np.array([target_radius] * 3),
                      rgb=np.asarray(target_rgba[:3], dtype=np.float64), label=SEG_TARGET, alpha=float(target_rgba[3])))
    return prims


def rays(view, fov, W, H, px, py):
    """Eye [3] and ray directions [M, 3] whose parameter is the eye depth along the view axis."""
    V = np.asarray(view, dtype=np.float64).reshape(4, 4)
    Rv, T = V[:3, :3], V[:3, 3]
    eye = -Rv.T @ T
    th = np.tan(np.radians(fov) / 2)
    ex = (2 * (np.asarray(px, dtype=np.float64) + 0.5) / W - 1) * th * W / H
    ey = (1 - 2 * (np.asarray(py, dtype=np.float64) + 0.5) / H) * th
    d_eye = np.stack([ex, ey, -np.ones_like(ex)], axis=1)
    return eye, d_eye @ Rv


def solid_interval(P, O, D):
    """(tn, tf) of the lines O + t D[m] (O [3] or [M, 3], D [M, 3]) against the solid P, a sphere, box or capped cylinder;
    tn > tf where the line misses it."""
    def slab(o, d, h):
        """Interval of t with |o + t d| <= h (one axis)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            a, b = (-h - o) / d, (h - o) / d
        inside = np.abs(o) <= h
        lo = np.where(d == 0, np.where(inside, -np.inf, np.inf), np.minimum(a, b))
        hi = np.where(d == 0, np.where(inside, np.inf, -np.inf), np.maximum(a, b))
        return lo, hi

    dl = D @ P["R"]                                                    # into the solid's frame
    o = np.broadcast_to((O - P["c"]) @ P["R"], dl.shape)
    if P["kind"] == SPHERE:
        a = np.einsum("ij,ij->i", dl, dl)
        with np.errstate(divide="ignore", invalid="ignore"):
            tc = -np.einsum("ij,ij->i", o, dl) / a
            v = o + tc[:, None] * dl
            disc = P["half"][0] ** 2 - np.einsum("ij,ij->i", v, v)
            half = np.sqrt(np.maximum(disc, 0) / a)
        ok = (a > 0) & (disc >= 0)                                     # (a = 0: a zero-length ray; a camera's rays have none)
        return np.where(ok, tc - half, np.inf), np.where(ok, tc + half, -np.inf)
    if P["kind"] == BOX:
        los, his = zip(*[slab(o[:, k], dl[:, k], P["half"][k]) for k in range(3)])
        return np.max(los, axis=0), np.min(his, axis=0)
    r, hl = P["half"][0], P["half"][2]                                # capped cylinder along local z
    a = dl[:, 0] ** 2 + dl[:, 1] ** 2
    par = a == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        tc = np.where(par, 0.0, -(o[:, 0] * dl[:, 0] + o[:, 1] * dl[:, 1]) / np.where(par, 1.0, a))
        vx, vy = o[:, 0] + tc * dl[:, 0], o[:, 1] + tc * dl[:, 1]
        disc = r * r - (vx * vx + vy * vy)
        half = np.where(par, np.inf, np.sqrt(np.maximum(disc, 0) / np.where(par, 1.0, a)))
    zlo, zhi = slab(o[:, 2], dl[:, 2], hl)
    return np.where(disc >= 0, np.maximum(tc - half, zlo), np.inf), np.where(disc >= 0, np.minimum(tc + half, zhi), -np.inf)


def intersect(P, eye, d):
    """(tn, tf) of every ray against primitive P; tn > tf where it misses."""
    if P["kind"] != PLANE:
        return solid_interval(P, eye, d)
    # pnr_render sees a plane as a surface, from both sides: tn = tf = t (pnr_ray_test's is the half-space below it, ray_ref.intersect)
    dn = d @ P["n"]
    on = (eye - P["c"]) @ P["n"]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(dn != 0, -on / np.where(dn != 0, dn, 1.0), np.inf)
    return t, np.where(dn != 0, t, -np.inf)


def normal_at(P, eye, d, t):
    """Outward world normals at the hit parameters t, and whether the hit lies on an edge (the face is undetermined)."""
    m = len(t)
    if P["kind"] == PLANE:
        return np.tile(P["n"], (m, 1)), np.zeros(m, bool)
    x = eye[None] + t[:, None] * d - P["c"][None]
    pl = x @ P["R"]
    if P["kind"] == SPHERE:
        return x, np.zeros(m, bool)
    if P["kind"] == BOX:
        s = np.abs(pl) / P["half"][None]
        k = np.argmax(s, axis=1)
        srt = np.sort(s, axis=1)
        edge = srt[:, 2] - srt[:, 1] <= 1e-5 * srt[:, 2]
        nl = np.zeros_like(pl)
        nl[np.arange(m), k] = pl[np.arange(m), k]
    else:
        rad = np.hypot(pl[:, 0], pl[:, 1])
        cap_s, side_s = np.abs(pl[:, 2]) / P["half"][2], rad / P["half"][0]
        cap = cap_s >= side_s
        edge = np.abs(cap_s - side_s) <= 1e-5 * np.maximum(cap_s, side_s)
        nl = np.where(cap[:, None], np.stack([0 * rad, 0 * rad, pl[:, 2]], 1), np.stack([pl[:, 0], pl[:, 1], 0 * rad], 1))
    return nl @ P["R"].T, edge


def _trace(prims, eye, d, near, far):
    """Per ray: every primitive's counted candidate depth [P, M] (inf where none) and the clip-proximity flag."""
    T = np.full((len(prims), len(d)), np.inf)
    clip = np.zeros(len(d), bool)
    for i, P in enumerate(prims):
        tn, tf = intersect(P, eye, d)
        hit = tn <= tf
        for t in (tn, tf):
            clip |= hit & np.isfinite(t) & ((np.abs(t - near) <= 1e-5 * near) | (np.abs(t - far) <= 1e-5 * far))
        t = np.where(tn > near, tn, tf)
        T[i] = np.where(hit & (t > near) & (t < far), t, np.inf)
    return T, clip


def _labels(prims, T):
    """(label, label behind the target) per ray."""
    opaque = np.array([P["alpha"] is None for P in prims])
    lab = np.array([P["label"] for P in prims])
    To = np.where(opaque[:, None], T, np.inf)
    io = np.argmin(To, axis=0)
    to = To[io, np.arange(T.shape[1])]
    behind = np.where(np.isfinite(to), lab[io], SEG_BACKGROUND)
    it = np.argmin(np.where(opaque[:, None], np.inf, T), axis=0)
    tt = T[it, np.arange(T.shape[1])]
    front = np.where(tt < to, SEG_TARGET, behind)
    return front, behind, io, to, it, tt


def render_pixels(q, target, px, py, view, fov, near, far, W, H, bodies=(), target_radius=0.2,
                  target_rgba=(1.0, 0.0, 0.0, 0.5), light_direction=(0.4, 0.2, 1.0), ambient=0.45, diffuse=0.55,
                  background=(1.0, 1.0, 1.0), data=None):
    """rgb [M, 3] uint8, depth [M], seg [M] uint8 and the ambiguity band [M] bool at the pixels (px[m], py[m]) of one env."""
    prims = scene_prims(q, target, target_radius, target_rgba, bodies, data)
    px, py = np.asarray(px, dtype=np.float64), np.asarray(py, dtype=np.float64)
    eye, d = rays(view, fov, W, H, px, py)
    T, clip = _trace(prims, eye, d, near, far)
    seg, behind, io, to, it, tt = _labels(prims, T)
    m = np.arange(len(px))
    light = np.asarray(light_direction, dtype=np.float64)
    light = light / np.linalg.norm(light)

    def shade(rgb, n, dd):
        n = n / np.linalg.norm(n, axis=1, keepdims=True)
        n = np.where((np.einsum("ij,ij->i", n, dd) > 0)[:, None], -n, n)
        k = ambient + diffuse * np.maximum(n @ light, 0.0)
        return np.clip(rgb * k[:, None], 0.0, 1.0)

    col = np.tile(np.asarray(background, dtype=np.float64), (len(px), 1))
    edge = np.zeros(len(px), bool)
    for i, P in enumerate(prims):
        sel = np.isfinite(to) & (io == i)
        if sel.any():
            n, e = normal_at(P, eye, d[sel], to[sel])
            col[sel] = shade(P["rgb"][None], n, d[sel])
            edge[sel] |= e
    depth = np.where(np.isfinite(to), to, np.inf)
    front = tt < to
    if front.any():
        P = prims[it[front][0]]
        n, _ = normal_at(P, eye, d[front], tt[front])
        a = P["alpha"]
        col[front] = a * shade(P["rgb"][None], n, d[front]) + (1 - a) * col[front]
        depth = np.where(front, tt, depth)
    rgb = np.floor(255 * col + 0.5).astype(np.uint8)

    # ambiguity band
    band = clip | edge
    for dx, dy in ((0.01, 0), (-0.01, 0), (0, 0.01), (0, -0.01)):
        e2, d2 = rays(view, fov, W, H, px + dx, py + dy)
        T2, _ = _trace(prims, e2, d2, near, far)
        s2, b2 = _labels(prims, T2)[:2]
        band |= (s2 != seg) | (b2 != behind)
    lab = np.array([P["label"] for P in prims])
    err = np.seterr(invalid="ignore")                                  # inf - inf where fewer than two candidates exist
    Ts = np.sort(T, axis=0)
    order = np.argsort(T, axis=0)
    first = lab[order[0]]
    for r in range(1, len(prims)):
        other = (lab[order[r]] != first) & np.isfinite(Ts[r]) & np.isfinite(Ts[0])
        close = other & (Ts[r] - Ts[0] <= 1e-5 * Ts[0])
        band |= close
    # among the opaque candidates too (the label behind the target)
    opaque = np.array([P["alpha"] is None for P in prims])
    To = np.sort(T[opaque], axis=0)
    oo = np.argsort(T[opaque], axis=0)
    lo = lab[opaque]
    for r in range(1, To.shape[0]):
        band |= (lo[oo[r]] != lo[oo[0]]) & np.isfinite(To[r]) & (To[r] - To[0] <= 1e-5 * To[0])
    np.seterr(**err)
    return dict(rgb=rgb, depth=depth, seg=seg.astype(np.uint8), band=band, behind=behind.astype(np.uint8))
