"""The inputs of the tests of the scene queries' per-env world (pnr_render_bodies, pnr_set_body_queries: the moving sphere in
pnr_render, pnr_ray_test and pnr_get_contacts), shared by the CPU tests (which assert on the float64 references that the GPU
comparisons cannot pass on nothing) and the GPU tests (which run the kernels on exactly these inputs).  Nothing here is a reference:
that is tests/scene_query_ref.py; its answers on these inputs are computed once here (render_reference, ray_reference,
contact_reference), shared by the tests and left unchanged.

Batches: N in SIZES = (3, 67): a partial wave, and more than one wave.  Env NO_SPHERE[N] of each batch has mass 0: no sphere.
Joints and targets are gpu_support.random_state's; the joint velocities are drawn here.  The caller's bodies are
gpu_support.coloured_bodies() (a rotated box, a sphere, the plane at z = -0.5) with a per-env offset on the box and the sphere
(body_positions); the plane stays where it is.  Radii and masses are per env.

Two placements of the moving sphere:
* "view" (render, rays): with the default camera a radius of 0.5 to 1.5 covers 0 to 8 pixels of a 33 x 17 image, and with a close
  camera random positions fall out of view; so the camera is CAMERA (30 units from the look-at point) and the centre lies 6 to 10
  units from the look-at point towards the eye, up to 1.5 aside, with a radius of 2.5 to 3.5: at least 20 pixels at 33 x 17.
* "touch" (contacts): the centre is one of the env's own sample centres plus an offset of U(0.6, 1.3) x (radius + sample radius)
  in a random direction, so about half the envs' chosen samples penetrate it, and it moves at up to 4 units/s per axis, so the
  law's damping term matters (kd 50 x a few units/s against kp 2000 x a depth of a few tenths).
"""
import functools

import numpy as np

import contact_query_ref as cq
import ray_ref as ry
import scene_query_ref as sref
import link_kinematics_ref as lk
from gpu_support import coloured_bodies, random_state

SIZES = (3, 67)
NO_SPHERE = {3: 1, 67: 40}
IMAGE_SIZES = ((83, 61), (33, 17))            # odd sizes: partial 16-byte chunks at the spans' ends
CAMERA = dict(camera_distance=30.0)
POINTER = 10
SEG_MOVING_BODY = 21
BODY_MOVING = 8                               # the sphere's body index in pnr_get_contacts
KP, KD, POINTER_RADIUS = 2000.0, 50.0, 0.2    # the configs' defaults
# the world rays see everything; the pointer's range sensor sees the bodies alone (the default mask: on its way to the sphere the
# arm itself would be in the way in one env of five)
RAY_MASKS = {"world": ry.HIT_ARM | ry.HIT_BODIES | ry.HIT_TARGET, "pointer": ry.HIT_BODIES}


def render_config(size):
    from pioneer_amd import RenderConfig
    return RenderConfig(render_width=size[0], render_height=size[1], **CAMERA)


def eye_direction():
    """unit vector from the camera's look-at point (the origin) to the eye, and two unit vectors across it"""
    from pioneer_amd import render
    V = np.asarray(render.view_matrix(render_config(IMAGE_SIZES[0])), dtype=np.float64).reshape(4, 4)
    eye = -V[:3, :3].T @ V[:3, 3]
    return eye / np.linalg.norm(eye), V[0, :3], V[1, :3]


@functools.lru_cache(maxsize=None)
def state(n):
    """q, qd [n, 6], targets [n, 3], float32"""
    q, tgt = random_state(n, 700 + n)
    qd = np.random.default_rng(710 + n).uniform(-2.0, 2.0, size=(n, 6)).astype(np.float32)
    return q, qd, tgt


def bodies():
    return coloured_bodies()


@functools.lru_cache(maxsize=None)
def body_positions(n):
    """[n, 3, 3] float32: the box and the sphere at their own positions plus an offset per env, the plane where it is"""
    rng = np.random.default_rng(720 + n)
    bp = np.tile(np.array([b.position for b, _ in bodies()], dtype=np.float64), (n, 1, 1))
    bp[:, 0:2] += rng.uniform((-3.0, -3.0, -1.0), (3.0, 3.0, 2.0), size=(n, 2, 3))
    return bp.astype(np.float32)


def shared_positions(n):
    return np.tile(np.array([b.position for b, _ in bodies()], dtype=np.float32), (n, 1, 1))


def _mass_radius(n, rng):
    mass = rng.uniform(0.5, 3.0, size=n)
    mass[NO_SPHERE[n]] = 0.0
    return mass, rng.uniform(2.5, 3.5, size=n)


@functools.lru_cache(maxsize=None)
def sphere_view(n):
    """body-state words [n, 8] float32 (position, velocity, mass, radius) of the "view" placement"""
    rng = np.random.default_rng(730 + n)
    u, right, up = eye_direction()
    mass, radius = _mass_radius(n, rng)
    x = (rng.uniform(6.0, 10.0, size=(n, 1)) * u + rng.uniform(-1.5, 1.5, size=(n, 1)) * right + rng.uniform(-1.5, 1.5, size=(n, 1)) * up)
    v = rng.uniform(-3.0, 3.0, size=(n, 3))
    return np.concatenate([x, v, mass[:, None], radius[:, None]], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sphere_touch(n):
    """.. of the "touch" placement"""
    rng = np.random.default_rng(740 + n)
    q, qd, _ = state(n)
    centres = cq.query(q, qd, ())["centres"]
    mass, radius = _mass_radius(n, rng)
    pick = rng.integers(0, cq.SAMPLES, size=n)
    sample_r = np.array([POINTER_RADIUS if r < 0 else r for _, _, r in cq.sample_table()])
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    x = centres[np.arange(n), pick] + (rng.uniform(0.6, 1.3, size=n) * (radius + sample_r[pick]))[:, None] * d
    v = rng.uniform(-4.0, 4.0, size=(n, 3))
    return np.concatenate([x, v, mass[:, None], radius[:, None]], axis=1).astype(np.float32)


def _aimed(n, start):
    """[n, 36, 6] float64 world rays: from start[k] through a 6 x 6 grid across env k's "view" sphere (+-1.6 radii), half as far again"""
    w = sphere_view(n).astype(np.float64)
    _, right, up = eye_direction()
    g = np.linspace(-1.6, 1.6, 6)
    gx, gy = (a.ravel() for a in np.meshgrid(g, g))
    aim = w[:, None, 0:3] + w[:, None, 7:8] * (gx[None, :, None] * right + gy[None, :, None] * up)
    frm = np.broadcast_to(start[:, None, :], aim.shape)
    return np.concatenate([frm, frm + 1.5 * (aim - frm)], axis=2)


@functools.lru_cache(maxsize=None)
def world_rays(n):
    """[n, 36, 6] float32 in the world frame, from a point near the eye"""
    u, right, up = eye_direction()
    return _aimed(n, np.tile(28.0 * u + 2.0 * up, (n, 1))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pointer_rays(n):
    """[n, 36, 6] float32 in the frame of env k's pointer link (a range sensor on the pointer): the same grid, from a point 0.3
    outside the pointer's sphere on its way to the moving sphere's centre"""
    q, _, _ = state(n)
    R, p, _, _ = lk.link_frames(q.astype(np.float64))
    R, p = R[:, POINTER], p[:, POINTER]
    to_sphere = sphere_view(n)[:, 0:3].astype(np.float64) - p
    start = p + 0.3 * to_sphere / np.linalg.norm(to_sphere, axis=1, keepdims=True)
    w = _aimed(n, start)
    local = lambda x: np.einsum("nji,nrj->nri", R, x - p[:, None])  # noqa: E731  (R^T (x - p))
    return np.concatenate([local(w[..., 0:3]), local(w[..., 3:6])], axis=2).astype(np.float32)


# ---- the references' answers on these inputs, once ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def render_reference(n, size):
    from pioneer_amd import render
    cfg = render_config(size)
    q, _, tgt = state(n)
    view = render.view_matrix(cfg)
    return [sref.render_env(q[k], tgt[k], cfg, view, bodies(), body_positions(n)[k], sphere_view(n)[k]) for k in range(n)]


@functools.lru_cache(maxsize=None)
def ray_reference(n, which):
    q, _, tgt = state(n)
    rays, parent = (world_rays(n), -1) if which == "world" else (pointer_rays(n), POINTER)
    return [sref.rays_env(q[k], tgt[k], rays[k], RAY_MASKS[which], bodies(), body_positions(n)[k], sphere_view(n)[k], parent)
            for k in range(n)]


def contact_bodies():
    make = {"plane": lambda b: cq.plane(b.size, b.position, b.orientation), "box": lambda b: cq.box(b.size, b.position, b.orientation),
            "sphere": lambda b: cq.sphere(b.size[0], b.position)}
    return tuple(make[b.shape](b) for b, _ in bodies())


@functools.lru_cache(maxsize=None)
def contact_reference(n, with_bodies=True, moving=True):
    q, qd, _ = state(n)
    w = sphere_touch(n)
    if not moving:
        w = w.copy()
        w[:, 3:6] = 0.0
    return sref.contacts(q, qd, contact_bodies() if with_bodies else (), body_positions(n) if with_bodies else None, w,
                         KP, KD, POINTER_RADIUS)
