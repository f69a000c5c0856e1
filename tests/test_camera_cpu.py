"""CPU tests of the per-env cameras (pnr_render_cameras / PioneerVectorEnv.render_frames(camera_link=..., cameras=...)): the host
helpers render.camera_pose and render.look_at_cameras against float64, and the float64 reference of tests/camera_ref.py on the
GPU test's own cases: it must leave enough of every checked image outside its ambiguity band for the bars of
tests/test_gpu_cameras.py to mean something, and the cameras must see what they are meant to see."""
import numpy as np
import pytest
import torch

import camera_cases as cc
import camera_ref as cr
import render_ref as rr


def _look_at(eye, target, up):
    """The float64 look-at: world -> eye view matrix of a camera at eye looking at target, up upwards in the image."""
    f = (target - eye) / np.linalg.norm(target - eye)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    V = np.eye(4)
    V[0, :3], V[1, :3], V[2, :3] = r, u, -f
    V[:3, 3] = -V[:3, :3] @ eye
    return V


def test_camera_pose_inverts_the_view_matrix():
    from pioneer_amd import RenderConfig, render
    cfgs = [RenderConfig(), RenderConfig(camera_distance=25.0, camera_yaw=-70.0, camera_pitch=-80.0, camera_roll=33.0),
            RenderConfig(camera_yaw=0.0, camera_pitch=0.0, camera_roll=0.0), RenderConfig(camera_yaw=180.0, camera_pitch=60.0, camera_roll=170.0,
                                                                                         camera_target=(3.0, -2.0, 1.0))]
    for cfg in cfgs:
        V = render.view_matrix(cfg)
        row = render.camera_pose(V)
        assert row.shape == (7,) and abs(np.linalg.norm(row[3:]) - 1.0) <= 1e-12
        assert np.abs(cr.views(np.zeros(6), None, row)[0] - V).max() <= 1e-12
    # every branch of the quaternion extraction: rotations by pi about x, y, z and the identity
    for quat in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (0.5, -0.5, -0.5, 0.5)):
        V = cr.views(np.zeros(6), None, np.r_[1.0, 2.0, 3.0, quat])[0]
        assert np.abs(cr.views(np.zeros(6), None, render.camera_pose(V))[0] - V).max() <= 1e-12


def test_look_at_cameras_agrees_with_a_float64_look_at():
    from pioneer_amd import render
    rng = np.random.default_rng(3)
    n = 200
    eye = rng.uniform(-40, 40, (n, 3))
    tgt = rng.uniform(-10, 10, (n, 3))
    eye[:4] = tgt[:4] + np.array([[30.0, 0, 0], [-30.0, 0, 1e-3], [0, -30.0, 0], [1.0, 1.0, 40.0]])      # along the axes, steeply down
    e32, t32 = eye.astype(np.float32), tgt.astype(np.float32)
    rows = render.look_at_cameras(torch.from_numpy(e32), torch.from_numpy(t32))
    assert rows.shape == (n, 7) and rows.dtype == torch.float32 and rows.device.type == "cpu"
    got = cr.views(np.zeros((n, 6)), None, rows.numpy().astype(np.float64))
    for k in range(n):
        want = _look_at(e32[k].astype(np.float64), t32[k].astype(np.float64), np.array([0.0, 0.0, 1.0]))
        assert np.abs(got[k, :3, :3] - want[:3, :3]).max() <= 1e-6, k
        assert np.abs(rows[k, :3].numpy() - e32[k]).max() == 0.0
    # one eye, one target, another up; array-likes are taken too
    one = render.look_at_cameras((10.0, 0.0, 5.0), (0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0))
    want = _look_at(np.array([10.0, 0.0, 5.0]), np.zeros(3), np.array([0.0, 1.0, 0.0]))
    assert one.shape == (1, 7) and np.abs(cr.views(np.zeros(6), None, one[0].numpy().astype(np.float64))[0] - want).max() <= 1e-5
    # [3] against [N, 3]
    many = render.look_at_cameras(torch.from_numpy(e32), (0.0, 0.0, 2.0))
    assert many.shape == (n, 7)


def test_look_at_cameras_refuses_a_view_along_up():
    from pioneer_amd import render
    with pytest.raises(ValueError):
        render.look_at_cameras((0.0, 0.0, 10.0), (0.0, 0.0, 1.0))
    with pytest.raises(ValueError):
        render.look_at_cameras(torch.tensor([[1.0, 2.0, 3.0], [5.0, 5.0, 5.0]]), torch.tensor([[0.0, 0.0, 0.0], [5.0, 5.0, 5.0]]))
    with pytest.raises(ValueError):
        render.look_at_cameras((3.0, 0.0, 0.0), (0.0, 0.0, 0.0), up=(-1.0, 0.0, 0.0))


@pytest.mark.parametrize("cam", cc.CAMERAS)
@pytest.mark.parametrize("size", cc.SIZES)
@pytest.mark.parametrize("n", cc.BATCHES)
def test_the_reference_leaves_the_gpu_cases_checkable(n, size, cam):
    """>= 0.9 of every checked env's pixels lie outside the band, the eye-shift rule included; and each of these cameras' world
    views goes through render.camera_pose and back to 1e-12 (the mounts turn the camera every way the arm can)."""
    from pioneer_amd import render
    c = cc.case(n, size, cam)
    V = cr.views(c["q"].astype(np.float64), c["link"], c["rows"].astype(np.float64))
    worst = 1.0
    for k in c["ks"]:
        assert np.abs(cr.views(np.zeros(6), None, render.camera_pose(V[k]))[0] - V[k]).max() <= 1e-12, k
        want = cc.case_reference(n, size, cam, k)
        share = float((~want["band"]).mean())
        worst = min(worst, share)
        assert share >= 0.9, f"env {k}: only {share:.3f} of the pixels are outside the band"
        assert (want["depth_bar"][np.isfinite(want["depth"])] > 0).all()
    print(f"{cam} n={n} {size}: worst share outside the band {worst:.3f}")


@pytest.mark.parametrize("cam", cc.CAMERAS)
def test_the_cameras_see_the_scene(cam):
    """Outside the band, over the 37-env cases: every camera sees the arm and a body in some image; the tracking camera, which looks
    at its env's target from 45 units (a target 0.4 wide, pixels about 1 wide there), has it in some image too."""
    labels = []
    for size in cc.SIZES:
        for k in cc.case(37, size, cam)["ks"]:
            want = cc.case_reference(37, size, cam, k)
            labels.append(set(np.unique(want["seg"][~want["band"]]).tolist()))
    seen = set().union(*labels)
    print(f"{cam}: labels {sorted(seen)}")
    assert any(rr.SEG_LINK0 < s < rr.SEG_TARGET for s in seen), "no arm in any image"
    assert any(s >= rr.SEG_BODY0 for s in seen), "no body in any image"
    if cam == "lookat":
        assert rr.SEG_TARGET in seen, "no target in any image"
