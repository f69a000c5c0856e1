"""CPU tests of pose inverse kinematics (pnr_solve_ik_pose): the float64 reference of tests/ik_pose_ref.py, its orientation error
against scipy, its convergence on every input set the GPU tests hold the kernel to, the float32 emulation of the law that gives
the GPU law-parity test its bound, and the C ABI surface that needs no device.  The GPU side is tests/test_gpu_ik_pose.py."""
import ctypes as C

import numpy as np
import pytest

import ik_pose_ref as ref

TOL = ref.DEFAULTS["tolerance"]
ANGLE_TOL = ref.DEFAULTS["angle_tolerance"]


def test_reference_orientation_error_against_scipy():
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(3)
    n = 512
    Ra, Rb = Rotation.random(n, random_state=1), Rotation.random(n, random_state=2)
    e, angle = ref.orientation_error(Ra.as_matrix(), Rb.as_matrix(), ref.FULL)
    want = (Rb * Ra.inv()).as_rotvec()                                    # R_target R^T, angle in [0, pi]
    assert np.abs(angle - np.linalg.norm(want, axis=1)).max() <= 1e-12
    ok = angle < 3.0                                                      # towards pi the axis is ill-conditioned in any form
    assert ok.sum() > 400 and np.abs(e[ok] - want[ok]).max() <= 1e-9
    # small rotations (where the solver stops): exact to rounding
    small = Rotation.from_rotvec(rng.normal(size=(n, 3)) * 1e-4)
    e, angle = ref.orientation_error(Ra.as_matrix(), (small * Ra).as_matrix(), ref.FULL)
    assert np.abs(e - small.as_rotvec()).max() <= 1e-12
    # AXIS mode: the rotation about u x v that takes u = R a to v = R_target a, whatever the roll about a
    a = np.array([0.3, -0.5, 0.8])
    a /= np.linalg.norm(a)
    e, angle = ref.orientation_error(Ra.as_matrix(), Rb.as_matrix(), ref.AXIS, 7.0 * a)     # any length
    u, v = Ra.apply(a), Rb.apply(a)
    assert np.abs(angle - np.arccos(np.clip((u * v).sum(axis=1), -1, 1))).max() <= 1e-7
    assert np.abs(Rotation.from_rotvec(e).apply(u) - v).max() <= 1e-9
    assert np.abs((e * u).sum(axis=1)).max() <= 1e-9 and np.abs(np.linalg.norm(e, axis=1) - angle).max() <= 1e-12
    roll = Rotation.from_rotvec(rng.uniform(-3, 3, size=(n, 1)) * a)
    e2, angle2 = ref.orientation_error(Ra.as_matrix(), (Rb * roll).as_matrix(), ref.AXIS, a)
    assert np.abs(e2 - e).max() <= 1e-9 and np.abs(angle2 - angle).max() <= 1e-9
    # where the axis cannot be formed the step is zero and finite, the angle pi
    eye = np.eye(3)[None]
    for mode in (ref.FULL, ref.AXIS):
        e, angle = ref.orientation_error(eye, np.diag([1.0, -1.0, -1.0])[None] if mode == ref.FULL else np.diag([-1.0, -1.0, 1.0])[None], mode)
        assert (e == 0).all() and abs(angle[0] - np.pi) <= 1e-12
    # quaternions: normalised by the reference, the sign does not matter, consistent with scipy (x, y, z, w)
    qt = Rb.as_quat()
    for scaled in (qt, -qt, 3.0 * qt):
        assert np.abs(ref.lk.matrix_from_quat(scaled) - Rb.as_matrix()).max() <= 1e-12


@pytest.mark.parametrize("n", ref.SIZES + [4096])
def test_reference_converges_for_every_env_of_the_shared_sets(n):
    """What makes "every env must converge" a fair demand of the kernel: the float64 law does, at every n and seed the GPU tests use
    (and at 4 096 poses: the basin the header quotes)."""
    lo, hi = ref.ik_ref.limits_f32()
    pos, quat, start, q_t = ref.near_set(n, ref.NEAR_SEED(n))
    assert (np.abs(q_t[:, 4]) >= 0.4).all() and np.abs(start - q_t).max() <= 0.2 + 1e-6
    q, dist, angle, its = ref.solve_ik_pose(pos, quat, start)
    print(f"NEAR n {n}: iterations {np.bincount(its)}, max distance {dist.max():.3g}, max angle {angle.max():.3g}")
    assert (dist <= TOL).all() and (angle <= ANGLE_TOL).all() and (its <= 8).all()
    assert (q >= lo).all() and (q <= hi).all()
    pos, quat = ref.point_set(n, ref.POINT_SEED(n))
    assert np.abs(ref.lk.matrix_from_quat(quat)[:, :, 0] - np.array([1.0, 0.0, 0.0])).max() <= 1e-6    # local x along world +x
    q, dist, angle, its = ref.solve_ik_pose(pos, quat, None, mode=ref.AXIS)
    print(f"POINT n {n}: iterations {np.bincount(its)} mean {its.mean():.2f}, max distance {dist.max():.3g}, max angle {angle.max():.3g}")
    assert (dist <= TOL).all() and (angle <= ANGLE_TOL).all() and (its <= 8).all()
    assert (q >= lo).all() and (q <= hi).all()
    # the pointer's x axis does point along +x (independent of orientation_error)
    _, R = ref.link_pose(q)
    assert (R[:, 0, 0] >= np.cos(ANGLE_TOL) - 1e-12).all()


def test_reference_from_the_rest_pose_to_full_poses_converges_for_a_share():
    """The rest pose is a wrist singularity and a full pose has branches: a share of FK poses is not reached from it."""
    pos, quat, q_t = ref.fk_set(2048, 1)
    q, dist, angle, its = ref.solve_ik_pose(pos, quat, None)
    ok = (dist <= TOL) & (angle <= ANGLE_TOL)
    away = np.abs(q_t[:, 4]) >= 0.4
    print(f"rest-pose starts on FK poses: {ok.mean():.4f} converge ({ok[away].mean():.4f} of the targets with |q5| >= 0.4), "
          f"iterations of those {np.bincount(its[ok])}")
    assert 0.5 < ok.mean() < 1.0
    assert (its[~ok] == 32).all()
    # out of reach in position, and an orientation the limits forbid at a reachable position: finite, inside the limits, all iterations
    lo, hi = ref.ik_ref.limits_f32()
    for p, qt in (((40.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)), ((18.0, 0.0, 4.0), (0.0, -1.0, 0.0, 1.0))):      # the pointer straight up, low in front of the base
        q, dist, angle, its = ref.solve_ik_pose([p], [qt])
        assert np.isfinite(q).all() and (q >= lo).all() and (q <= hi).all() and its[0] == 32
        assert dist[0] > TOL or angle[0] > ANGLE_TOL


def test_float32_emulation_of_the_law_stays_close_to_float64():
    """The deviation a correct float32 implementation of the law shows on the law-parity inputs (damping 0.1, error_damping 0.01:
    the better-conditioned setting), per case over the NEAR sets of every size: tests/test_gpu_ik_pose.py allows the kernel 4 x
    this, at most 1e-3 rad.  Measured: 3.2e-5 / 5.6e-5 (1 iteration, FULL / AXIS), 9.2e-5 / 3.1e-4 (3 iterations), 3.6e-6 /
    7.7e-6 (rest start, the envs that start less than 3 rad from the target's orientation).  At the default damping 0.03 three iterations deviate by up to 2.6e-3 rad in AXIS mode: the free roll
    leaves a direction that only lambda^2 holds."""
    for name, its, mode, near in ref.law_cases():
        dev = ref.law_deviation(its, mode, near)
        print(f"{name}: float32 emulation deviates by {dev:.3g} rad; bound for the kernel {min(4 * dev, 1e-3):.3g}")
        assert 0 < dev <= 1e-3                       # steps are up to 0.5 rad: float32 rounding is orders below the law
    pos, quat, start, _ = ref.near_set(1000, ref.NEAR_SEED(1000))
    kw = dict(max_iterations=3, tolerance=0.0, angle_tolerance=0.0, mode=ref.AXIS)
    dev = np.abs(ref.solve_ik_pose(pos, quat, start, **kw)[0] - ref.solve_ik_pose(pos, quat, start, dtype=np.float32, **kw)[0]).max()
    print(f"default damping, 3 iterations, AXIS: {dev:.3g} rad")
    # the float32 chain walk itself: the existing FK bound
    q = np.random.default_rng(0).uniform(-1, 1, (64, 6)) * ref.LIMITS
    for link, local in ((10, None), (7, (0.3, -0.2, 0.5)), (4, None)):
        p, R, J = ref.kinematics_f32(q.astype(np.float32), link, local)
        p64, R64 = ref.link_pose(q.astype(np.float32), link, local)
        assert np.abs(p - p64).max() <= 3e-5 and np.abs(R - R64).max() <= 2e-6
        assert np.abs(J - ref.ik_ref.jacobian(q.astype(np.float32), link, local)).max() <= 6e-5


def test_library_surface_without_a_device(hip_lib):
    from pioneer_amd import _lib
    p = _lib.PnrIkPoseParams()
    assert hip_lib.pnr_ik_pose_params_default(p) == 0
    assert p.struct_size == C.sizeof(_lib.PnrIkPoseParams) == 112              # the header's struct, as the library compiled it
    assert (p.link, p.max_iterations, p.mode) == (10, 32, _lib.IK_ORIENT_FULL) and _lib.IK_ORIENT_AXIS == 1
    assert tuple(p.local_point) == (0.0, 0.0, 0.0) and tuple(p.local_axis) == (1.0, 0.0, 0.0)
    got = {k: getattr(p, k) for k in ref.DEFAULTS}
    assert got == ref.DEFAULTS, got                                              # the reference's defaults are the library's
    assert hip_lib.pnr_ik_pose_params_default(None) == -1
    buf = (C.c_float * 36)()
    vp = C.cast(buf, C.c_void_p)
    assert hip_lib.pnr_solve_ik_pose(None, p, None, vp, None, vp, None, None, None, None) == -1
    assert b"null handle" in hip_lib.pnr_last_error(None)
    # the Python layers carry the call
    from pioneer_amd import PioneerKinematicEnv, PioneerVectorEnv
    assert callable(PioneerVectorEnv.solve_ik_pose) and callable(PioneerKinematicEnv.solve_ik_pose)
