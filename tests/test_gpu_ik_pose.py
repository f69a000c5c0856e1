"""GPU tests of pnr_solve_ik_pose (PioneerVectorEnv.solve_ik_pose and the façade's) against the independent float64 reference of
tests/ik_pose_ref.py: the solver held to the stated law at fixed iteration counts, convergence of every pose of the shared NEAR
and POINT sets (tests/test_ik_pose_cpu.py proves the reference converges on each), a start at the target, poses out of reach,
the independence of an env's result from the batch around it, argument checking, graph capture, the façade."""
import ctypes as C

import numpy as np
import pytest
import torch

import ik_pose_ref as ref

pytestmark = pytest.mark.gpu

SIZES = ref.SIZES
FK_TOL = 3e-5            # the existing forward-kinematics bound (test_gpu_link_states.py)
ANG_TOL = 2e-6           # the existing quaternion bound: per component of the link's unit quaternion
# The angle between the kernel's float32 rotation and the float64 one: a rotation by the small angle d moves the quaternion's
# components by d / 2 in norm, each component is within ANG_TOL, so d <= 2 sqrt(4) ANG_TOL = 4 ANG_TOL; the target's float32
# quaternion is normalised and squared into a matrix by the kernel in float32 (another few 1e-7).  8 ANG_TOL covers both.
ANGLE_EVAL_TOL = 8 * ANG_TOL
TOL, ANGLE_TOL = ref.DEFAULTS["tolerance"], ref.DEFAULTS["angle_tolerance"]
UP_LOW = ((18.0, 0.0, 4.0), (0.0, -1.0, 0.0, 1.0))        # the pointer straight up, low in front of the base: not reached
FAR = ((40.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0))            # the links' lengths add up to 30.07


def host_tensor(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def solve(env, quat, pos, start=None, **kw):
    return [t.cpu().numpy() for t in env.solve_ik_pose(host_tensor(quat), host_tensor(pos), host_tensor(start), **kw)]


def check_converged(env, q, res, ang, its, pos, quat, mode, want_its):
    """Checks 2 and 3 of the suite: the returned joints, evaluated by the float64 chain, are at the target pose; the kernel's own
    residuals agree with that evaluation; no more than one iteration beyond the reference; inside the limits."""
    dist, angle = ref.pose_error(q, pos, quat, mode)
    print(f"n {len(q)}: max distance {dist.max():.3g}, max angle {angle.max():.3g}, iterations {np.bincount(its)}, "
          f"reference {np.bincount(want_its)}; residual_out off by {np.abs(res - dist).max():.3g}, angle_out by {np.abs(ang - angle).max():.3g}")
    assert (dist <= TOL + 2 * FK_TOL).all()
    assert (angle <= ANGLE_TOL + ANGLE_EVAL_TOL).all()
    assert np.abs(res - dist).max() <= 2 * FK_TOL
    assert np.abs(ang - angle).max() <= ANGLE_EVAL_TOL
    assert (its <= want_its + 1).all()          # one float32 distance or angle may land on the other side of its tolerance
    assert (q >= env.r_lo).all() and (q <= env.r_hi).all()


@pytest.mark.parametrize("n", SIZES)
def test_fixed_iteration_counts_follow_the_stated_law(n):
    """tolerance = angle_tolerance = 0: every env runs exactly the asked iterations and its joints are the float64 law's within
    4 x the deviation of the float32 emulation of the law on the same input sets (tests/ik_pose_ref.py law_deviation; two
    correct float32 implementations order their sums differently), at most 1e-3 rad: steps are up to 0.5 rad, any other law is
    off by orders of magnitude.  damping 0.1 / error_damping 0.01, the better-conditioned setting.  Joints are compared for the
    envs whose start is less than 3 rad from the target's orientation (all NEAR starts; from the rest pose 88-91 % of the poses
    in FULL mode, 99.5 % in AXIS mode): towards half a turn the rotation axis is ill-conditioned in any number format (forming
    R_target in float32 alone moves the first step of the env 2.5e-4 rad from half a turn by 6e-5 rad; the kernel: 5.6e-5).
    The others must stay finite and inside the limits.
    Emulation deviation -> bound, and the kernel's error on an MI355X (largest over the four sizes), per case:
    1 iteration, NEAR start: FULL 3.2e-5 -> 1.3e-4, kernel 1.9e-5; AXIS 5.6e-5 -> 2.3e-4, kernel 9.7e-5;
    3 iterations, NEAR start: FULL 9.2e-5 -> 3.7e-4, kernel 1.1e-4; AXIS 3.1e-4 -> 1e-3 (the cap), kernel 2.4e-4;
    1 iteration, rest start: FULL 3.6e-6 -> 1.4e-5, kernel 3.4e-6; AXIS 7.7e-6 -> 3.1e-5, kernel 1.2e-5."""
    from pioneer_amd import PioneerVectorEnv
    env = PioneerVectorEnv(n, device="cuda:0", seed=1)
    for name, iters, mode, near in ref.law_cases():
        pos, quat, start, want, _, held = ref.law_reference(n, iters, mode, near)
        bound = min(4 * ref.law_deviation(iters, mode, near), 1e-3)
        q, res, ang, its = solve(env, quat, pos, start, max_iterations=iters, align_axis=(1, 0, 0) if mode == ref.AXIS else None,
                                 **ref.LAW_PARAMS)
        assert held.all() if near else held.mean() >= 0.85                       # what is compared is nearly all of the set
        err = np.abs(q.astype(np.float64) - want)[held].max() if held.any() else 0.0
        print(f"n {n}, {name}: joint error {err:.3g}, bound {bound:.3g} ({held.sum()} of {n} envs start below "
              f"{ref.MAX_START_ANGLE} rad; the others are off by {np.abs(q - want)[~held].max() if not held.all() else 0:.3g})")
        assert err <= bound
        assert np.isfinite(q).all() and (q >= env.r_lo).all() and (q <= env.r_hi).all()
        assert (its == iters).all()
        dist, angle = ref.pose_error(q, pos, quat, mode)
        assert np.abs(res - dist).max() <= 2 * FK_TOL and np.abs(ang - angle).max() <= ANGLE_EVAL_TOL
    env.close()


@pytest.mark.parametrize("n", SIZES)
def test_every_near_pose_converges_with_the_defaults(n):
    from pioneer_amd import PioneerVectorEnv
    env = PioneerVectorEnv(n, device="cuda:0", seed=2)
    pos, quat, start, _ = ref.near_set(n, ref.NEAR_SEED(n))
    out = env.solve_ik_pose(host_tensor(quat), host_tensor(pos), host_tensor(start))
    assert [tuple(t.shape) for t in out] == [(n, 6), (n,), (n,), (n,)]
    assert [t.dtype for t in out] == [torch.float32, torch.float32, torch.float32, torch.int32]
    q, res, ang, its = (t.cpu().numpy() for t in out)
    want_its = ref.solve_ik_pose(pos, quat, start)[3]
    check_converged(env, q, res, ang, its, pos, quat, ref.FULL, want_its)
    env.close()


@pytest.mark.parametrize("n", SIZES)
def test_every_point_target_converges_in_axis_mode_from_the_rest_pose(n):
    """The roll about the axis is free: only the position and the axis angle are asserted."""
    from pioneer_amd import PioneerVectorEnv
    env = PioneerVectorEnv(n, device="cuda:0", seed=3)
    pos, quat = ref.point_set(n, ref.POINT_SEED(n))
    q, res, ang, its = solve(env, quat, pos, align_axis=(1.0, 0.0, 0.0))
    want_its = ref.solve_ik_pose(pos, quat, None, mode=ref.AXIS)[3]
    check_converged(env, q, res, ang, its, pos, quat, ref.AXIS, want_its)
    # the same through the env's own targets (target=None) and an axis of another length
    env.reset(target_positions=host_tensor(pos))
    q2, res2, ang2, its2 = solve(env, quat, None, align_axis=(2.5, 0.0, 0.0))
    assert np.array_equal(q, q2) and np.array_equal(res, res2) and np.array_equal(ang, ang2) and np.array_equal(its, its2)
    env.close()


def test_a_start_at_the_target_pose_is_returned_bit_for_bit():
    from pioneer_amd import PioneerVectorEnv
    n = 200
    env = PioneerVectorEnv(n, device="cuda:0", seed=4)
    start = (np.random.default_rng(8).uniform(-0.9, 0.9, size=(n, 6)) * ref.LIMITS).astype(np.float32)
    pos, quat = ref.fk_pose(start)
    for kw in ({}, {"align_axis": (0.0, 0.0, 1.0)}):
        q, res, ang, its = solve(env, quat.astype(np.float32), pos.astype(np.float32), start, **kw)
        assert np.array_equal(q.view(np.uint32), start.view(np.uint32)) and (its == 0).all()
        assert (res <= 2 * FK_TOL).all() and (ang <= ANGLE_EVAL_TOL).all()
    env.close()


def test_poses_out_of_reach():
    from pioneer_amd import PioneerVectorEnv
    n = 130
    env = PioneerVectorEnv(n, device="cuda:0", seed=5)
    rng = np.random.default_rng(12)
    far_quat = rng.normal(size=(n // 2, 4))                                       # any orientation
    pos = np.concatenate([np.tile(FAR[0], (n // 2, 1)), np.tile(UP_LOW[0], (n - n // 2, 1))]).astype(np.float32)
    quat = np.concatenate([far_quat, np.tile(UP_LOW[1], (n - n // 2, 1))]).astype(np.float32)
    for iters in (32, 5):
        q, res, ang, its = solve(env, quat, pos, max_iterations=iters)
        assert np.isfinite(q).all() and np.isfinite(res).all() and np.isfinite(ang).all()
        assert (q >= env.r_lo).all() and (q <= env.r_hi).all()
        assert (its == iters).all()
        dist, angle = ref.pose_error(q, pos, quat)
        assert np.abs(res - dist).max() <= 2 * FK_TOL and np.abs(ang - angle).max() <= ANGLE_EVAL_TOL
        assert (res[:n // 2] >= 9.9).all()
        assert ((res[n // 2:] > TOL) | (ang[n // 2:] > ANGLE_TOL)).all()
    env.close()


def test_an_envs_result_does_not_depend_on_the_batch_around_it():
    from pioneer_amd import PioneerVectorEnv
    n = 1000
    rng = np.random.default_rng(31)
    pos, quat, start, _ = ref.near_set(n, 77)
    pos, quat, start = pos.copy(), quat.copy(), start.copy()
    bad = rng.random(n) < 0.2                                                   # mixed with poses that are not reached
    pos[bad] = np.where(rng.random((bad.sum(), 1)) < 0.5, np.float32(FAR[0]), np.float32(UP_LOW[0]))
    quat[bad & (pos[:, 0] == 18.0)] = UP_LOW[1]
    start[rng.random(n) < 0.3] = 0.0                                            # and with rest-pose starts
    env = PioneerVectorEnv(n, device="cuda:0", seed=2)
    base = [t.cpu() for t in env.solve_ik_pose(host_tensor(quat), host_tensor(pos), host_tensor(start))]
    assert len(np.unique(base[3].numpy())) >= 4                                 # the lanes of a wave stop at different times
    perm = rng.permutation(n)
    moved = [t.cpu() for t in env.solve_ik_pose(host_tensor(quat[perm]), host_tensor(pos[perm]), host_tensor(start[perm]))]
    for a, b in zip(base, moved):
        assert torch.equal(a[torch.from_numpy(perm)], b)
    env.close()
    one = PioneerVectorEnv(1, device="cuda:0", seed=2)
    its = base[3].numpy()
    slow = int(np.argmax(np.where(its < 32, its, -1)))                          # the slowest env that did converge
    for k in (0, 63, 64, 517, 999, slow, int(np.argmax(its))):
        alone = [t.cpu() for t in one.solve_ik_pose(host_tensor(quat[k:k + 1]), host_tensor(pos[k:k + 1]), host_tensor(start[k:k + 1]))]
        for a, b in zip(base, alone):
            assert torch.equal(a[k:k + 1], b), k
    one.close()


def test_bad_arguments_are_refused_and_leave_the_output_alone():
    from pioneer_amd import PioneerVectorEnv, PnrError, _lib
    n = 37
    env = PioneerVectorEnv(n, device="cuda:0", seed=4)
    lib, h, st = env.lib, env._h, env._stream()
    q = torch.full((n * 6 + 4,), -7.25, dtype=torch.float32, device=env.device)
    res = torch.full((n + 2,), -7.25, dtype=torch.float32, device=env.device)
    ang = torch.full((n + 2,), -7.25, dtype=torch.float32, device=env.device)
    its = torch.full((n + 2,), -7, dtype=torch.int32, device=env.device)
    pos_np, quat_np, start_np, _ = ref.near_set(n, ref.NEAR_SEED(n))
    tgt, quat, start = host_tensor(pos_np).cuda(), host_tensor(quat_np).cuda(), host_tensor(start_np).cuda()
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731

    def params(**kw):
        p = _lib.PnrIkPoseParams()
        assert lib.pnr_ik_pose_params_default(p) == 0
        for k, v in kw.items():
            if k in ("local_point", "local_axis"):
                for i in range(3):
                    getattr(p, k)[i] = v[i]
            else:
                setattr(p, k, v)
        return p

    def call(p, tgt_=P(tgt), quat_=P(quat), qi=P(start), q_=P(q), res_=P(res), ang_=P(ang), its_=P(its), handle=h):
        return lib.pnr_solve_ik_pose(handle, p, tgt_, quat_, qi, q_, res_, ang_, its_, st)

    def refused(rc, word):
        assert rc == -1
        assert word in lib.pnr_last_error(h), lib.pnr_last_error(h)

    nan, inf = float("nan"), float("inf")
    assert call(params(), handle=None) == -1 and b"null handle" in lib.pnr_last_error(None)
    refused(call(None), b"null params")
    refused(call(params(), q_=None), b"null q_out")
    refused(call(params(), quat_=None), b"null target_quat")
    refused(call(params(struct_size=64)), b"struct_size")
    for link in (-1, 11):
        refused(call(params(link=link)), b"link")
    for mode in (-1, 2):
        refused(call(params(mode=mode)), b"mode")
    for it in (0, 1025, -3):
        refused(call(params(max_iterations=it)), b"max_iterations")
    for bad in (0.0, -1.0, nan, inf):
        for name in ("damping", "max_step", "orientation_weight"):
            refused(call(params(**{name: bad})), name.encode())
    for bad in (-1e-9, nan, inf):
        for name in ("error_damping", "tolerance", "angle_tolerance"):
            refused(call(params(**{name: bad})), b"pnr_solve_ik_pose: " + name.encode())
    refused(call(params(local_point=(0.0, nan, 0.0))), b"local_point")
    for axis in ((0.0, 0.0, 0.0), (0.0, inf, 0.0), (nan, 1.0, 0.0)):
        refused(call(params(mode=1, local_axis=axis)), b"local_axis")
    refused(call(params(), q_=P(q, 4)), b"aligned")
    for name in ("tgt_", "quat_", "qi", "res_", "ang_", "its_"):
        buf = {"tgt_": tgt, "quat_": quat, "qi": start, "res_": res, "ang_": ang, "its_": its}[name]
        refused(call(params(), **{name: P(buf, 2)}), b"aligned")
    refused(call(params(), tgt_=None), b"before the first pnr_reset")              # the env's own target before the first reset
    with pytest.raises(PnrError, match="before the first pnr_reset"):
        env.solve_ik_pose(quat)
    with pytest.raises(PnrError, match="local_axis"):
        env.solve_ik_pose(quat, tgt, align_axis=(0.0, 0.0, 0.0))
    torch.cuda.synchronize()
    assert (q == -7.25).all() and (res == -7.25).all() and (ang == -7.25).all() and (its == -7).all()
    # .. and the same buffers are written by a good call, nothing past n * 6 floats (n floats, n ints)
    assert call(params()) == 0
    torch.cuda.synchronize()
    assert (q[:n * 6] != -7.25).all() and (q[n * 6:] == -7.25).all()
    assert (res[:n] <= 1e-3).all() and (ang[:n] >= 0).all() and (ang[:n] <= 1e-3).all() and (its[:n] >= 1).all()
    assert (res[n:] == -7.25).all() and (ang[n:] == -7.25).all() and (its[n:] == -7).all()
    # NULL optional outputs and a NULL start are accepted
    keep = q.clone()
    assert call(params(), res_=None, ang_=None, its_=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(q, keep)
    assert call(params(), qi=None, res_=None, ang_=None, its_=None) == 0
    # a NaN target: a non-finite residual for that env only, no error, no hang
    tgt[0, 1] = nan
    _, r2, a2, i2 = env.solve_ik_pose(quat, tgt, start)
    assert not np.isfinite(float(r2[0])) and int(i2[0]) == 32 and bool(torch.isfinite(r2[1:]).all()) and bool((r2[1:] <= 1e-3).all())
    assert bool(torch.isfinite(a2[1:]).all())
    env.close()


def test_graph_capture_replays_the_eager_result():
    from pioneer_amd import PioneerVectorEnv
    n = 64
    env = PioneerVectorEnv(n, device="cuda:0", seed=6)
    pos, quat, start, _ = ref.near_set(n, 5)
    pos, quat, start = host_tensor(pos).cuda(), host_tensor(quat).cuda(), host_tensor(start).cuda()
    out = {"q": torch.empty((n, 6), device=env.device), "residual": torch.empty(n, device=env.device),
           "angle": torch.empty(n, device=env.device), "iterations": torch.empty(n, dtype=torch.int32, device=env.device)}
    s = torch.cuda.Stream(device=env.device)
    s.wait_stream(torch.cuda.current_stream(env.device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        env.solve_ik_pose(quat, pos, start, out=out)                              # warm-up on the capture stream
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            env.solve_ik_pose(quat, pos, start, out=out)
    torch.cuda.synchronize()
    pos2, quat2, start2, _ = ref.near_set(n, 6)
    pos.copy_(host_tensor(pos2)); quat.copy_(host_tensor(quat2)); start.copy_(host_tensor(start2))
    for t in out.values():
        t.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    eager = env.solve_ik_pose(quat, pos, start)
    for a, b in zip(out.values(), eager):
        assert torch.equal(a, b)
    assert bool((out["residual"] <= 1e-3).all()) and bool((out["angle"] <= 1e-3).all()) and bool((out["iterations"] >= 1).all())
    env.close()


def test_facade_solve_ik_pose_puts_the_pointer_on_the_target_with_the_orientation():
    from pioneer_amd import PioneerKinematicEnv, PioneerVectorEnv
    env = PioneerKinematicEnv()
    target = (18.5, -3.25, 4.5)
    env.reset_world(target_position=target)
    # pointing: the pointer's x axis along world +x at the env's own target
    q, residual, angle = env.solve_ik_pose((0.0, 0.0, 0.0, 1.0), align_axis=(1.0, 0.0, 0.0))
    assert q.shape == (6,) and q.dtype == np.float64 and residual <= TOL and angle <= ANGLE_TOL
    env.reset_world(joint_positions=q, target_position=target)
    rec = env._vec.link_states()[0, 10].double().cpu().numpy()                   # position[3], quaternion (x, y, z, w)
    assert np.linalg.norm(rec[0:3] - np.array(target)) <= TOL + 2 * FK_TOL
    x_axis = ref.lk.matrix_from_quat(rec[3:7])[:, 0]
    assert np.arccos(min(1.0, x_axis[0])) <= ANGLE_TOL + ANGLE_EVAL_TOL
    # a full pose: that of known joints, asked at its position; the link's quaternion comes back (either sign)
    q_t = np.array([[0.4, 0.5, -0.3, 0.2, 0.8, -0.1]])
    pos, quat = ref.fk_pose(q_t)
    q, residual, angle = env.solve_ik_pose(quat[0], target_position=pos[0])
    assert residual <= TOL and angle <= ANGLE_TOL
    env.reset_world(joint_positions=q)
    rec = env._vec.link_states()[0, 10].double().cpu().numpy()
    assert np.linalg.norm(rec[0:3] - pos[0]) <= TOL + 2 * FK_TOL
    assert min(np.abs(rec[3:7] - quat[0]).max(), np.abs(rec[3:7] + quat[0]).max()) <= ANGLE_TOL / 2 + 4 * ANG_TOL
    # solve_ik still returns what the vector env's solve_ik returns
    env.reset_world(target_position=target)
    q1, r1 = env.solve_ik()
    vec = PioneerVectorEnv(1, device="cuda:0", seed=0)
    q2, r2, _ = vec.solve_ik(torch.tensor([target]))
    assert np.array_equal(q1, q2[0].double().cpu().numpy()) and r1 == float(r2[0].item())
    q3, r3 = env.solve_ik(target_position=(16.0, 5.0, 3.0))
    q4, r4, _ = vec.solve_ik(torch.tensor([[16.0, 5.0, 3.0]]))
    assert np.array_equal(q3, q4[0].double().cpu().numpy()) and r3 == float(r4[0].item())
    vec.close()
    env.close()
