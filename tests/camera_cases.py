"""The camera cases that tests/test_camera_cpu.py (the reference alone) and tests/test_gpu_cameras.py (the engine against it)
share: three mounts, the batch sizes, the image sizes, the seeds and the envs that are checked."""
import functools

import numpy as np

import camera_ref as cr
import render_ref as rr
from gpu_support import coloured_bodies, random_state

CAMERAS = ("pointer", "arm2", "lookat")
SIZES = ((48, 32), (41, 29))
BATCHES = (1, 37, 1000)
NEAR, FAR = 0.05, 200.0
POINTER_MOUNT = (0.0, 0.0, 0.3, 1.0, 0.0, 0.0, 0.0)                 # outside the pointer's sphere (radius 0.2), looking along the link's +z
ARM2_MOUNT = (2.0, 1.0, 2.5, 0.5, -0.5, -0.5, 0.5)
ARM2_LINK, POINTER_LINK = 4, 10


def with_body_positions(n, size, cam):
    """the one case whose bodies get a world position per env"""
    return (n, tuple(size), cam) == (37, (41, 29), "arm2")


def checked_envs(n):
    return list(range(n)) if n <= 37 else sorted({0, n - 1, *np.random.default_rng(n).choice(n, 10, replace=False).tolist()})


def ref_bodies(bodies, positions=None):
    """render_ref's body tuples of [(SceneBody, rgba)], body b at positions[b] where given"""
    return [(b.shape, b.position if positions is None else tuple(map(float, positions[i])), b.orientation, b.size, rgba)
            for i, (b, rgba) in enumerate(bodies)]


@functools.lru_cache(maxsize=None)
def case(n, size, cam):
    """One parity case: the envs' joints and targets (float32), the mount (link or None, float32 camera rows [7] or [n, 7]), the
    projection, the per-env body positions (float32 [n, 3, 3] or None) and the envs to check."""
    from pioneer_amd import render
    q, tgt = random_state(n, 1000 * n + 10 * size[0] + CAMERAS.index(cam))
    rng = np.random.default_rng(7 * n + size[1] + CAMERAS.index(cam))
    fov = 60.0
    if cam == "pointer":
        link, rows = POINTER_LINK, np.asarray(POINTER_MOUNT, dtype=np.float32)
    elif cam == "arm2":                                               # a row per env: the mount, its position and (unnormalised) quaternion jittered
        rows = np.asarray(ARM2_MOUNT, dtype=np.float64) + np.concatenate([rng.uniform(-0.05, 0.05, (n, 3)), rng.uniform(-0.02, 0.02, (n, 4))], axis=1)
        link, rows = ARM2_LINK, (rows * rng.uniform(0.5, 2.0, (n, 1)) ** np.r_[0, 0, 0, 1, 1, 1, 1]).astype(np.float32)
    else:                                                             # a tracking camera: 45 units from each env's target, looking at it
        az = rng.uniform(-np.pi, np.pi, n)
        el = rng.uniform(0.2, 0.9, n)
        away = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1)
        link, fov = None, 40.0
        rows = render.look_at_cameras((tgt.astype(np.float64) + 45.0 * away).astype(np.float32), tgt).numpy()
    bodies = coloured_bodies()
    bp = None
    if with_body_positions(n, size, cam):
        base = np.array([b.position for b, _ in bodies], dtype=np.float64)
        bp = (base[None] + rng.uniform(-1.0, 1.0, (n, len(bodies), 3)) * np.array([3.0, 3.0, 0.3])).astype(np.float32)
    return dict(n=n, size=tuple(size), cam=cam, q=q, tgt=tgt, link=link, rows=rows, fov=fov, near=NEAR, far=FAR, bodies=bodies,
                body_positions=bp, ks=checked_envs(n))


@functools.lru_cache(maxsize=None)
def case_reference(n, size, cam, k):
    """reference(case(n, size, cam), k), computed once and left unchanged"""
    return reference(case(n, size, cam), k)


def reference(c, k, q=None):
    """camera_ref.reference_env of env k of case c (q: other joints than the case's own, [6])"""
    W, H = c["size"]
    rows = c["rows"] if c["rows"].ndim == 1 else c["rows"][k]
    qk = c["q"][k] if q is None else q
    view = cr.views(qk.astype(np.float64), c["link"], rows.astype(np.float64))[0]
    bodies = ref_bodies(c["bodies"], None if c["body_positions"] is None else c["body_positions"][k])
    return cr.reference_env(qk, c["tgt"][k], view, c["fov"], c["near"], c["far"], W, H, bodies, c["link"] is not None, data=_visuals())


@functools.lru_cache(maxsize=None)
def _visuals():
    return rr.load_visuals()
