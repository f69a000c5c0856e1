"""CPU tests of the link-state query (pnr_get_link_states / PioneerVectorEnv.link_states / Item.pose() on link items): the
float64 reference of tests/link_kinematics_ref.py checked against itself and the renderer's chain, the C ABI surface, and the
façade's Pose / Velocity types.  The GPU side is tests/test_gpu_link_states.py."""
import ctypes as C
import os
import re

import numpy as np

import link_kinematics_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_joints(n, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    lim = np.array([3.1416, 1.309, 1.309, 3.1416, 1.5708, 3.1416])
    return rng.uniform(-scale * lim, scale * lim, size=(n, 6)), rng.uniform(-3.0, 3.0, size=(n, 6))


def test_reference_origins_match_the_renderer_chain():
    from pioneer_amd import render
    q, qd = _random_joints(64, 1, scale=1.3)
    _, p, _, _ = ref.link_frames(q, qd)
    for i in range(len(q)):
        np.testing.assert_allclose(p[i], render.link_origins(q[i])[1:], rtol=0, atol=1e-12)


def test_reference_link_order_is_the_urdf_joint_order():
    import pioneer_amd
    from pioneer_amd import model
    chain = ref.load_chain()
    assert tuple(j["child"] for j in chain) == pioneer_amd.LINK_NAMES == tuple(model.LINKS[1:])
    assert len(pioneer_amd.LINK_NAMES) == 11
    # the record convention rests on this: link frame = COM frame, fixed joints do not rotate
    import json
    links = json.load(open(ref.GOLDEN))["links"]
    assert all(list(links[name]["inertial_xyz"]) == [0, 0, 0] for name in pioneer_amd.LINK_NAMES)
    assert all(list(j["rpy"]) == [0, 0, 0] for j in chain)


def test_reference_quaternions_match_its_rotation_matrices():
    q, qd = _random_joints(200, 2, scale=1.5)
    R, _, _, _ = ref.link_frames(q, qd)
    rec = ref.link_states(q, qd)
    quat = rec[..., 3:7].reshape(-1, 4)
    assert np.all(quat[:, 3] >= 0)
    np.testing.assert_allclose(np.linalg.norm(quat, axis=1), 1.0, atol=1e-14)
    np.testing.assert_allclose(ref.matrix_from_quat(quat), R.reshape(-1, 3, 3), rtol=0, atol=1e-12)
    # link 0 is static: identity at the origin, no velocity
    np.testing.assert_array_equal(rec[:, 0], np.tile([0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0], (len(q), 1)))


def test_reference_velocities_are_derivatives_of_its_poses():
    q, qd = _random_joints(50, 3, scale=1.2)
    h = 1e-6
    _, _, v, w = ref.link_frames(q, qd)
    Rp, pp, _, _ = ref.link_frames(q + h * qd, qd)
    Rm, pm, _, _ = ref.link_frames(q - h * qd, qd)
    v_fd = (pp - pm) / (2 * h)
    dR = (Rp - Rm) / (2 * h)
    R0, _, _, _ = ref.link_frames(q, qd)
    W = dR @ np.swapaxes(R0, -1, -2)                       # skew(omega) = dR/dt R^T
    w_fd = np.stack([W[..., 2, 1], W[..., 0, 2], W[..., 1, 0]], axis=-1)
    np.testing.assert_allclose(v, v_fd, rtol=0, atol=1e-6 * (1 + np.abs(v).max()))
    np.testing.assert_allclose(w, w_fd, rtol=0, atol=1e-6 * (1 + np.abs(w).max()))
    assert np.abs(v[:, 1:]).max() > 1.0 and np.abs(w[:, 1:]).max() > 1.0      # the check is not vacuous


def test_link_state_entry_point_is_declared_and_exported(hip_lib):
    from pioneer_amd import _lib
    assert "pnr_get_link_states" in _lib.SIGNATURES
    assert hasattr(hip_lib, "pnr_get_link_states")
    header = open(os.path.join(ROOT, "include", "pioneer_amd.h")).read()
    assert re.search(r"^#define PNR_NUM_LINKS 11\b", header, re.M)
    assert re.search(r"^#define PNR_LINK_STATE_DIM 13\b", header, re.M)
    assert re.search(r"int pnr_get_link_states\(pnr_handle h, const float\* joint_state, float\* out, void\* stream\);", header)
    assert (_lib.NUM_LINKS, _lib.LINK_STATE_DIM, _lib.ABI_VERSION) == (11, 13, 5)


def test_link_state_null_handle_is_invalid_without_a_device(hip_lib):
    buf = (C.c_float * 16)()
    assert hip_lib.pnr_get_link_states(None, None, C.cast(buf, C.c_void_p), None) == -1         # PNR_ERR_INVALID
    assert b"null handle" in hip_lib.pnr_last_error(None)


def test_pose_is_a_two_tuple_with_xyz_and_rpy():
    from pioneer_amd.scene import Item, Pose, Scene, Velocity
    p = Pose((1.0, 2.0, 3.0), Scene.rpy2quat((0.3, -0.2, 1.1)))
    pos, orn = p
    assert pos == (1.0, 2.0, 3.0) and p.xyz == pos and p.position == pos and p.orientation == orn
    np.testing.assert_allclose(p.rpy, (0.3, -0.2, 1.1), atol=1e-12)
    item = Item("box", "box", (1, 2, 3), (0, 0, 0, 1), True, (1, 1, 1))
    pos, orn = item.pose()
    assert isinstance(item.pose(), Pose) and pos == (1.0, 2.0, 3.0) and orn == (0.0, 0.0, 0.0, 1.0)
    vel = item.velocity()
    assert isinstance(vel, Velocity) and vel.linear == (0.0, 0.0, 0.0) and vel.angular == (0.0, 0.0, 0.0)
