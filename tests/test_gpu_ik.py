"""GPU tests of pnr_get_jacobian / pnr_solve_ik (PioneerVectorEnv.jacobian, solve_ik, target_reachable and the façade's
solve_ik) against the independent float64 reference of tests/ik_ref.py: the Jacobian for every joint source, the solver held
to the stated iteration law at fixed iteration counts, convergence on the reachable inner box, out-of-reach targets, the
independence of an env's result from the batch around it, argument checking, graph capture."""
import ctypes as C

import numpy as np
import pytest
import torch

import ik_ref
import link_kinematics_ref as lk
from gpu_support import LIMITS, dyn_joints, kin_joints

pytestmark = pytest.mark.gpu

SIZES = [1, 37, 64, 1000]
LOCAL_POINT = (0.3, -0.2, 0.5)
INNER_LO, INNER_HI = (15.0, -8.0, 2.0), (22.0, 8.0, 6.0)
FK_TOL = 3e-5            # the existing forward-kinematics bound (test_gpu_link_states.py)
LIN_TOL = 2 * FK_TOL     # a linear entry is built from the difference of two positions
ANG_TOL = 2e-6           # the existing quaternion bound


def inner_targets(n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = np.array(INNER_LO), np.array(INNER_HI)
    return (lo + (hi - lo) * rng.random((n, 3))).astype(np.float32)


def check_jacobians(env, q, qd, joint_state=None):
    """Every link of {10, 7, 4, 0} with and without a local point against the reference, the zero columns, and J qd against
    the velocities link_states() reports for the same joints."""
    n = env.num_envs
    q64, qd64 = np.asarray(q, dtype=np.float64), np.asarray(qd, dtype=np.float64)
    rec = env.link_states(joint_state).cpu().numpy().astype(np.float64)
    body_joints = {10: 6, 7: 5, 4: 3, 0: 0}                                     # joints between the base and the link
    for link in (10, 7, 4, 0):
        for local in (LOCAL_POINT, None):
            J = env.jacobian(link, local, joint_state)
            assert J.shape == (n, 6, 6) and J.dtype == torch.float32 and J.device == env.device
            J = J.cpu().numpy()
            want = ik_ref.jacobian(q64, link, local)
            lin, ang = np.abs(J[:, 0:3] - want[:, 0:3]).max(), np.abs(J[:, 3:6] - want[:, 3:6]).max()
            print(f"n {n} link {link} local {local}: linear error {lin:.3g}, angular error {ang:.3g}")
            assert lin <= LIN_TOL and ang <= ANG_TOL
            assert (J[:, :, body_joints[link]:] == 0.0).all()
            if local is None:
                v = (J.astype(np.float64) @ qd64[:, :, None])[:, :, 0]
                for rows, lo, tol in ((slice(0, 3), 7, 2e-5), (slice(3, 6), 10, 2e-6)):
                    exp = rec[:, link, lo:lo + 3]
                    bound = tol * (1.0 + np.linalg.norm(exp, axis=-1))
                    assert (np.abs(v[:, rows] - exp).max(axis=-1) <= bound).all(), (link, lo)


@pytest.mark.parametrize("n", SIZES)
def test_jacobian_of_a_kinematic_handles_own_state(n):
    from pioneer_amd import PioneerVectorEnv
    env = PioneerVectorEnv(n, device="cuda:0", seed=3 + n)
    env.reset()
    g = torch.Generator(device="cpu").manual_seed(n)
    amax = torch.from_numpy(env.a_max)
    for _ in range(4):
        env.vector_step(((torch.rand(n, 6, generator=g) * 2 - 1) * amax).cuda())
    q, qd = kin_joints(env)
    check_jacobians(env, q, qd)
    # the raw call writes exactly N x 36 floats: the rest of an oversized buffer keeps its sentinel
    want = env.jacobian(10, LOCAL_POINT).cpu().reshape(-1)
    big = torch.full((n * 36 + 1000,), -7.25, dtype=torch.float32, device=env.device)
    lp = (C.c_double * 3)(*LOCAL_POINT)
    assert env.lib.pnr_get_jacobian(env._h, None, 10, lp, C.c_void_p(big.data_ptr()), env._stream()) == 0
    torch.cuda.synchronize()
    big = big.cpu()
    assert torch.equal(big[:n * 36], want)
    assert (big[n * 36:] == -7.25).all()
    env.close()


@pytest.mark.parametrize("mode", ["kinematic", "dynamic"])
@pytest.mark.parametrize("n", SIZES)
def test_jacobian_of_a_callers_joint_buffer(mode, n):
    from pioneer_amd import EngineConfig, PioneerVectorEnv
    env = PioneerVectorEnv(n, device="cuda:0", seed=11, engine_config=EngineConfig(mode=mode))
    rng = np.random.default_rng(n)
    q = rng.uniform(-1.0, 1.0, size=(n, 6)).astype(np.float32) * LIMITS
    qd = rng.uniform(-3.0, 3.0, size=(n, 6)).astype(np.float32)
    js = torch.from_numpy(np.concatenate([q, qd], axis=1)).cuda()
    keep = js.clone()
    check_jacobians(env, q, qd, js)                                               # no reset needed: pure kinematics
    assert torch.equal(js, keep)                                                  # only read
    env.close()


@pytest.mark.parametrize("n", SIZES)
def test_jacobian_of_a_dynamics_handles_simulated_joints(n):
    from pioneer_amd import EngineConfig, PioneerVectorEnv, SimulationConfig
    env = PioneerVectorEnv(n, device="cuda:0", seed=5, simulation_config=SimulationConfig(gravity=9.81),
                           engine_config=EngineConfig(mode="dynamic"))
    env.reset()
    d = env.get_dyn_state()
    rng = np.random.default_rng(7 + n)
    d[0:6] = torch.from_numpy((rng.uniform(-0.9, 0.9, size=(n, 6)).astype(np.float32) * LIMITS).T.copy()).cuda()
    d[6:12] = torch.from_numpy(rng.uniform(-2.0, 2.0, size=(6, n)).astype(np.float32)).cuda()
    env.set_dyn_state(d)
    for _ in range(5):
        env.world_step()
    q, qd = dyn_joints(env)
    assert np.isfinite(q).all()
    check_jacobians(env, q, qd)
    env.close()


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_fixed_iteration_counts_follow_the_stated_law(n, iters):
    """tolerance 0: every env runs exactly `iters` iterations, and its joints are the reference law's to 1e-4 rad (float32
    rounding moves them by a few 1e-6; steps are up to 0.5 rad, so any other law is off by orders of magnitude)."""
    from pioneer_amd import PioneerVectorEnv
    env = PioneerVectorEnv(n, device="cuda:0", seed=1)
    targets = inner_targets(n, 100 + n)
    rng = np.random.default_rng(200 + n)
    starts = rng.uniform(-0.3, 0.3, size=(n, 6)).astype(np.float32)
    for q_init in (None, starts):
        q, res, its = env.solve_ik(torch.from_numpy(targets), None if q_init is None else torch.from_numpy(q_init),
                                   max_iterations=iters, tolerance=0.0)
        want, want_res, _ = ik_ref.solve_ik(targets, q_init, max_iterations=iters, tolerance=0.0)
        err = np.abs(q.cpu().numpy().astype(np.float64) - want).max()
        print(f"n {n} iterations {iters} start {'rest' if q_init is None else 'given'}: joint error {err:.3g}")
        assert err <= 1e-4
        assert (its.cpu().numpy() == iters).all()
        assert np.abs(res.cpu().numpy() - want_res).max() <= 1e-2                # |d residual| <= |J| |dq| ~ 60 x 1e-4
    env.close()


@pytest.mark.parametrize("n", SIZES)
def test_every_inner_box_target_converges_from_the_rest_pose(n):
    from pioneer_amd import PioneerKinematicConfig, PioneerVectorEnv
    env = PioneerVectorEnv(n, device="cuda:0", seed=17 + n, pioneer_config=PioneerKinematicConfig(target_lo=INNER_LO, target_hi=INNER_HI))
    env.reset()
    q, res, its = env.solve_ik()
    assert q.shape == (n, 6) and q.dtype == torch.float32 and res.shape == (n,) and res.dtype == torch.float32
    assert its.shape == (n,) and its.dtype == torch.int32
    q, res, its = q.cpu().numpy(), res.cpu().numpy(), its.cpu().numpy()
    targets = env.state_dict()["target"].astype(np.float64)
    assert (targets >= np.array(INNER_LO)).all() and (targets <= np.array(INNER_HI)).all()
    dist = np.linalg.norm(targets - ik_ref.point_position(q.astype(np.float64)), axis=1)
    _, _, want_its = ik_ref.solve_ik(targets)
    print(f"n {n}: max distance {dist.max():.3g}, iterations {np.bincount(its)}, reference {np.bincount(want_its)}")
    assert (dist <= 1e-3 + 2 * FK_TOL).all()
    assert np.abs(res - dist).max() <= 2 * FK_TOL
    assert (its <= want_its + 1).all()                     # one float32 distance may land on the other side of the tolerance
    assert (q >= env.r_lo).all() and (q <= env.r_hi).all()
    assert env.target_reachable().all()
    env.close()


def test_targets_out_of_reach():
    from pioneer_amd import PioneerVectorEnv
    n = 1000
    env = PioneerVectorEnv(n, device="cuda:0", seed=9)
    far = torch.tensor([40.0, 0.0, 0.0]).repeat(n, 1)
    env.reset(target_positions=far)
    q, res, its = (t.cpu().numpy() for t in env.solve_ik())
    assert np.isfinite(q).all() and np.isfinite(res).all()
    assert (res >= 9.9).all() and (its == 32).all()        # the links' lengths add up to 30.07
    assert (q >= env.r_lo).all() and (q <= env.r_hi).all()
    reach = env.target_reachable()
    assert reach.dtype == torch.bool and reach.shape == (n,) and not reach.any()
    # the reference's own target box holds both kinds (the float64 reference: about 97 % reachable)
    env.reset()
    share = float(env.target_reachable().float().mean())
    print(f"reachable share of the default target box, {n} envs: {share:.4f}")
    assert 0.9 < share < 1.0
    env.close()


def test_an_envs_result_does_not_depend_on_the_batch_around_it():
    from pioneer_amd import PioneerVectorEnv
    n = 1000
    rng = np.random.default_rng(31)
    lo, hi = np.array([15.0, -10.0, 2.0]), np.array([25.0, 10.0, 6.0])       # the default box: reachable and unreachable targets
    targets = (lo + (hi - lo) * rng.random((n, 3))).astype(np.float32)
    starts = rng.uniform(-0.3, 0.3, size=(n, 6)).astype(np.float32)
    env = PioneerVectorEnv(n, device="cuda:0", seed=2)
    base = [t.cpu() for t in env.solve_ik(torch.from_numpy(targets), torch.from_numpy(starts))]
    assert len(np.unique(base[2].numpy())) >= 3                                # the lanes of a wave stop at different times
    # moved to another lane (and another wave)
    perm = rng.permutation(n)
    moved = [t.cpu() for t in env.solve_ik(torch.from_numpy(targets[perm]), torch.from_numpy(starts[perm]))]
    for a, b in zip(base, moved):
        assert torch.equal(a[torch.from_numpy(perm)], b)
    env.close()
    # solved alone
    one = PioneerVectorEnv(1, device="cuda:0", seed=2)
    slow = int(np.argmax(base[2].numpy()))
    for k in (0, 63, 64, 517, 999, slow):
        alone = [t.cpu() for t in one.solve_ik(torch.from_numpy(targets[k:k + 1]), torch.from_numpy(starts[k:k + 1]))]
        for a, b in zip(base, alone):
            assert torch.equal(a[k:k + 1], b), k
    one.close()


def test_bad_arguments_are_refused_and_leave_the_output_alone():
    from pioneer_amd import PioneerVectorEnv, PnrError, _lib
    n = 37
    env = PioneerVectorEnv(n, device="cuda:0", seed=4)
    lib, h, st = env.lib, env._h, env._stream()
    q = torch.full((n * 6 + 4,), -7.25, dtype=torch.float32, device=env.device)
    res = torch.full((n,), -7.25, dtype=torch.float32, device=env.device)
    its = torch.full((n,), -7, dtype=torch.int32, device=env.device)
    jac = torch.full((n * 36 + 4,), -7.25, dtype=torch.float32, device=env.device)
    tgt = torch.from_numpy(inner_targets(n, 1)).cuda()
    js = torch.zeros((n, 12), dtype=torch.float32, device=env.device)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731

    def params(**kw):
        p = _lib.PnrIkParams()
        assert lib.pnr_ik_params_default(p) == 0
        for k, v in kw.items():
            if k == "local_point":
                for i in range(3):
                    p.local_point[i] = v[i]
            else:
                setattr(p, k, v)
        return p

    def refused(rc, word):
        assert rc == -1
        assert word in lib.pnr_last_error(h), lib.pnr_last_error(h)

    nan, inf = float("nan"), float("inf")
    refused(lib.pnr_solve_ik(h, None, P(tgt), None, P(q), P(res), P(its), st), b"null params")
    refused(lib.pnr_solve_ik(h, params(), P(tgt), None, None, P(res), P(its), st), b"null q_out")
    refused(lib.pnr_solve_ik(h, params(struct_size=12), P(tgt), None, P(q), P(res), P(its), st), b"struct_size")
    for link in (-1, 11):
        refused(lib.pnr_solve_ik(h, params(link=link), P(tgt), None, P(q), P(res), P(its), st), b"link")
    for it in (0, 1025, -3):
        refused(lib.pnr_solve_ik(h, params(max_iterations=it), P(tgt), None, P(q), P(res), P(its), st), b"max_iterations")
    for bad in (0.0, -1.0, nan, inf):
        refused(lib.pnr_solve_ik(h, params(damping=bad), P(tgt), None, P(q), P(res), P(its), st), b"damping")
        refused(lib.pnr_solve_ik(h, params(max_step=bad), P(tgt), None, P(q), P(res), P(its), st), b"max_step")
    for bad in (-1e-9, nan, inf):
        refused(lib.pnr_solve_ik(h, params(tolerance=bad), P(tgt), None, P(q), P(res), P(its), st), b"tolerance")
    refused(lib.pnr_solve_ik(h, params(local_point=(0.0, nan, 0.0)), P(tgt), None, P(q), P(res), P(its), st), b"local_point")
    refused(lib.pnr_solve_ik(h, params(), P(tgt), None, P(q, 4), P(res), P(its), st), b"aligned")
    refused(lib.pnr_solve_ik(h, params(), P(tgt, 2), None, P(q), P(res), P(its), st), b"aligned")
    # the env's own target / joints before the first reset
    refused(lib.pnr_solve_ik(h, params(), None, None, P(q), P(res), P(its), st), b"before the first pnr_reset")
    refused(lib.pnr_get_jacobian(h, None, 10, None, P(jac), st), b"before the first pnr_reset")
    with pytest.raises(PnrError, match="before the first pnr_reset"):
        env.solve_ik()
    with pytest.raises(PnrError, match="before the first pnr_reset"):
        env.jacobian()
    refused(lib.pnr_get_jacobian(h, P(js), 10, None, None, st), b"null out")
    for link in (-1, 11):
        refused(lib.pnr_get_jacobian(h, P(js), link, None, P(jac), st), b"link")
    refused(lib.pnr_get_jacobian(h, P(js), 10, (C.c_double * 3)(0.0, inf, 0.0), P(jac), st), b"local_point")
    refused(lib.pnr_get_jacobian(h, P(js), 10, None, P(jac, 4), st), b"aligned")
    refused(lib.pnr_get_jacobian(h, P(js, 4), 10, None, P(jac), st), b"aligned")
    assert lib.pnr_solve_ik(None, params(), P(tgt), None, P(q), P(res), P(its), st) == -1
    assert lib.pnr_get_jacobian(None, P(js), 10, None, P(jac), st) == -1
    torch.cuda.synchronize()
    assert (q == -7.25).all() and (res == -7.25).all() and (its == -7).all() and (jac == -7.25).all()
    # .. and the same buffers are written by a good call
    assert lib.pnr_solve_ik(h, params(), P(tgt), None, P(q), P(res), P(its), st) == 0
    assert lib.pnr_get_jacobian(h, P(js), 10, None, P(jac), st) == 0
    torch.cuda.synchronize()
    assert (q[:n * 6] != -7.25).all() and (q[n * 6:] == -7.25).all() and (res <= 1e-3).all() and (its >= 1).all()
    assert (jac[n * 36:] == -7.25).all() and (jac[:n * 36] != -7.25).all()
    # non-finite targets: non-finite residuals, no error, no hang
    tgt[0, 1] = nan
    _, r2, i2 = env.solve_ik(tgt)
    assert not np.isfinite(float(r2[0])) and int(i2[0]) == 32 and bool(torch.isfinite(r2[1:]).all())
    env.close()


def test_graph_capture_replays_the_eager_result():
    from pioneer_amd import PioneerVectorEnv
    n = 64
    env = PioneerVectorEnv(n, device="cuda:0", seed=6)
    env.reset()
    tgt = torch.from_numpy(inner_targets(n, 5)).cuda()
    out = {"q": torch.empty((n, 6), device=env.device), "residual": torch.empty(n, device=env.device),
           "iterations": torch.empty(n, dtype=torch.int32, device=env.device)}
    jac = torch.empty((n, 6, 6), device=env.device)
    s = torch.cuda.Stream(device=env.device)
    s.wait_stream(torch.cuda.current_stream(env.device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        env.solve_ik(tgt, out=out)                                              # warm-up on the capture stream
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            env.solve_ik(tgt, out=out)
            env.jacobian(7, LOCAL_POINT, out=jac)
    torch.cuda.synchronize()
    tgt.copy_(torch.from_numpy(inner_targets(n, 6)))
    for t in (*out.values(), jac):
        t.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    eager = env.solve_ik(tgt)
    assert torch.equal(out["q"], eager[0]) and torch.equal(out["residual"], eager[1]) and torch.equal(out["iterations"], eager[2])
    assert torch.equal(jac, env.jacobian(7, LOCAL_POINT))
    assert bool((out["residual"] <= 1e-3).all())
    env.close()


def test_facade_solve_ik_puts_the_pointer_on_the_target():
    from pioneer_amd import PioneerKinematicEnv
    env = PioneerKinematicEnv()
    target = (18.5, -3.25, 4.5)
    env.reset_world(target_position=target)
    q, residual = env.solve_ik()
    assert q.shape == (6,) and q.dtype == np.float64 and residual <= 1e-3
    env.reset_world(joint_positions=q, target_position=target)
    obs = env.observe()
    assert np.linalg.norm(obs[126:129] - np.array(target)) <= 1e-3 + 2 * FK_TOL
    assert obs[135] <= 1e-3 + 2 * FK_TOL
    q2, _ = env.solve_ik(target_position=(16.0, 5.0, 3.0))
    assert np.linalg.norm(ik_ref.point_position(q2[None])[0] - np.array([16.0, 5.0, 3.0])) <= 1e-3 + 2 * FK_TOL
    env.close()
