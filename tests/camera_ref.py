"""float64 test support of pnr_render_cameras (PioneerVectorEnv.render_frames(camera_link=..., cameras=...)): the view matrix of
every env's camera from the URDF chain, and the bars a frame is held to.

It reads nothing of the engine: the parent link's frame is link_kinematics_ref.link_frames' (tests/golden/urdf_chain.json), the
camera row's rotation is matrix_from_quat's, and the pixels come from render_ref.render_pixels, which takes any view.

The bars are test_gpu_render.check_env's: labels equal outside the ambiguity band, rgb within 1, the same pixels infinite, depth
within 1e-4 relative.  A link-mounted camera changes one of them, the depth bar: the eye and the surface it sees are each a
float32 world position that the project bars at bars.POS_TOL, so their relative position is off by some d with |d| <= 2 POS_TOL
per axis, and the depth moves linearly with it.  The reference is therefore rendered six more times, the eye shifted by
+-2 POS_TOL along x, y and z; a pixel's depth may be off by 1e-4 depth + sum over the axes of max |depth_shifted - depth|, and a
pixel whose label (in front of or behind the target) changes under a shift joins the band.  World-frame cameras get rows already
rounded to float32 on both sides and keep the plain 1e-4 depth.
"""
import numpy as np

import link_kinematics_ref as lk
import render_ref as rr
from bars import POS_TOL

EYE_SHIFT = 2.0 * POS_TOL


def views(q, link, cameras):
    """World -> eye view matrices [N, 4, 4] of the cameras `cameras` ([7] or [N, 7]: position | quaternion x, y, z, w of the camera
    frame in its parent frame; x right, y up, looking along -z) mounted on link `link` (0 .. 10, link_frames' order) of the envs
    whose joints are q [N, 6]; link None or -1: the parent frame is the world."""
    q = np.atleast_2d(np.asarray(q, dtype=np.float64))
    n = q.shape[0]
    cam = np.broadcast_to(np.asarray(cameras, dtype=np.float64), (n, 7))
    Rc, pc = lk.matrix_from_quat(cam[:, 3:7]), cam[:, 0:3]
    if link is None or link < 0:
        Rp, pp = np.broadcast_to(np.eye(3), (n, 3, 3)), np.zeros((n, 3))
    else:
        R, p, _, _ = lk.link_frames(q)
        Rp, pp = R[:, link], p[:, link]
    Rw = Rp @ Rc                                                   # camera -> world: its columns are right, up, back
    pw = pp + np.einsum("nij,nj->ni", Rp, pc)
    V = np.zeros((n, 4, 4))
    V[:, :3, :3] = np.transpose(Rw, (0, 2, 1))
    V[:, :3, 3] = -np.einsum("nji,nj->ni", Rw, pw)
    V[:, 3, 3] = 1.0
    return V


def reference_env(q, tgt, view, fov, near, far, W, H, bodies, link_mounted, data=None):
    """render_ref.render_pixels at every pixel of one env's image, with `depth_bar` [W H] and, for a link-mounted camera, the band
    widened by the eye-shift rule of the module docstring."""
    yy, xx = np.mgrid[0:H, 0:W]
    px, py = xx.ravel(), yy.ravel()
    view = np.asarray(view, dtype=np.float64)
    data = data or rr.load_visuals()
    render = lambda V: rr.render_pixels(np.asarray(q, dtype=np.float64), np.asarray(tgt, dtype=np.float64), px, py, V, fov, near,  # noqa: E731
                                        far, W, H, bodies=bodies, data=data)
    want = render(view)
    with np.errstate(invalid="ignore"):
        bar = 1e-4 * np.where(np.isfinite(want["depth"]), want["depth"], 0.0)
        if link_mounted:
            band = want["band"].copy()
            for axis in range(3):
                worst = np.zeros(len(px))
                for sign in (1.0, -1.0):
                    V = view.copy()
                    V[:3, 3] -= sign * EYE_SHIFT * view[:3, axis]            # the eye moved by sign * EYE_SHIFT along the world axis
                    moved = render(V)
                    band |= (moved["seg"] != want["seg"]) | (moved["behind"] != want["behind"])
                    both = np.isfinite(moved["depth"]) & np.isfinite(want["depth"])
                    worst = np.maximum(worst, np.where(both, np.abs(moved["depth"] - want["depth"]), 0.0))
                bar = bar + worst
            want["band"] = band
    want["depth_bar"] = bar
    return want


def check_env(frames, k, want, what=""):
    """Env k of the engine's frames (numpy rgb, depth, seg) against reference_env's `want`.  Returns, and prints, the worst ratio
    of a depth error to its bar."""
    seg = frames["seg"][k].reshape(-1)
    rgb = frames["rgb"][k].reshape(-1, 3).astype(np.int32)
    dep = frames["depth"][k].reshape(-1).astype(np.float64)
    ok = ~want["band"]
    bad = ok & (seg != want["seg"])
    assert not bad.any(), f"{what} env {k}: {bad.sum()} labels differ outside the band, e.g. pixels {np.argwhere(bad)[:5].ravel()}"
    same = ok & (seg == want["seg"])
    worst_rgb = np.abs(rgb[same] - want["rgb"][same].astype(np.int32)).max(initial=0)
    assert worst_rgb <= 1, f"{what} env {k}: rgb off by {worst_rgb}"
    assert np.array_equal(np.isinf(dep[same]), np.isinf(want["depth"][same])), f"{what} env {k}: other pixels are infinite"
    fin = same & np.isfinite(want["depth"])
    ratio = float((np.abs(dep[fin] - want["depth"][fin]) / want["depth_bar"][fin]).max(initial=0.0))
    print(f"{what} env {k}: worst depth error / bar = {ratio:.3f}")
    assert ratio <= 1.0, f"{what} env {k}: a depth error is {ratio:.3f} of its bar"
    return ratio
