"""GPU tests of pnr_solve_ik_multi (PioneerVectorEnv.solve_ik_multi, the façade's starts= / q_ref=) against the float64 reference
of tests/ik_multi_ref.py: the per-start law at S = 1 held to the existing laws' bounds, a start's independence of S, the selection
checked exactly on the kernel's own per-start outputs, convergence against the reference, independence of the batch, refusals,
graph capture, the façade."""
import ctypes as C

import numpy as np
import pytest
import torch

import ik_multi_ref as ref
import ik_pose_ref as pref
import ik_ref

pytestmark = pytest.mark.gpu

SIZES = pref.SIZES                                   # 1, 37, 64, 1000
SHAPES = [(n, S) for n in SIZES for S in (1, 8, 16)] + [(37, 2), (37, 32), (37, 64)]    # partial last waves, the row crossing, the shift edge
FK_TOL, ANG_TOL = 3e-5, 2e-6                         # the existing bounds (test_gpu_ik_pose.py)
ANGLE_EVAL_TOL = 8 * ANG_TOL
TOL, ANGLE_TOL = pref.DEFAULTS["tolerance"], pref.DEFAULTS["angle_tolerance"]
MAX_IT = 32
WEIGHT = 10.0
TASKS = (ref.POSITION, ref.POSE, ref.AXIS)
FAR = ((40.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0))      # the links' lengths add up to 30.07
UP_LOW = ((18.0, 0.0, 4.0), (0.0, -1.0, 0.0, 1.0))  # the pointer straight up, low in front of the base: not reached


def T(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def solve(env, task, pos, quat, **kw):
    """solve_ik_multi of one task as numpy arrays."""
    if task == ref.AXIS:
        kw["align_axis"] = (1.0, 0.0, 0.0)
    for key in ("starts", "q_init", "q_ref"):
        if isinstance(kw.get(key), np.ndarray):
            kw[key] = T(kw[key])
    out = env.solve_ik_multi(None if task == ref.POSITION else T(quat), T(pos), **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def mixed_poses(n, seed, bad_share=0.2):
    """FULL-set poses mixed with poses that are not reached: float32 (pos, quat)."""
    pos, quat, _ = pref.fk_set(n, seed)
    pos, quat = pos.copy(), quat.copy()
    rng = np.random.default_rng(seed + 1)
    bad = rng.random(n) < bad_share
    far = rng.random(n) < 0.5
    pos[bad & far], pos[bad & ~far] = np.float32(FAR[0]), np.float32(UP_LOW[0])
    quat[bad & ~far] = np.float32(UP_LOW[1])
    return pos, quat


def within(task, res, ang):
    """The kernel's convergence test on its own float32 outputs."""
    ok = res <= np.float32(TOL)
    return ok if task == ref.POSITION else ok & (ang <= np.float32(ANGLE_TOL))


@pytest.mark.parametrize("n", SIZES)
def test_one_start_follows_the_stated_laws(n):
    """The fixed-iteration cases of the two single-start laws through solve_ik_multi(starts=1, q_init=...), held to the existing
    tests' bounds: the pose law to 4 x the float32 emulation's deviation, at most 1e-3 rad, on the held envs
    (test_gpu_ik_pose.py); the position law to 1e-4 rad (test_gpu_ik.py); the kernel's residuals to the FK / angle evaluation
    tolerances."""
    from pioneer_amd import PioneerVectorEnv
    env = PioneerVectorEnv(n, device="cuda:0", seed=1)
    for name, iters, mode, near in pref.law_cases():
        pos, quat, start, want, _, held = pref.law_reference(n, iters, mode, near)
        bound = min(4 * pref.law_deviation(iters, mode, near), 1e-3)
        for policy in ("best", "first"):
            out = solve(env, ref.AXIS if mode == pref.AXIS else ref.POSE, pos, quat, starts=1, q_init=start, max_iterations=iters, policy=policy,
                        **pref.LAW_PARAMS)
            q = out["q"]
            assert held.all() if near else held.mean() >= 0.85
            err = np.abs(q.astype(np.float64) - want)[held].max() if held.any() else 0.0
            print(f"n {n}, {name}, {policy}: joint error {err:.3g}, bound {bound:.3g}")
            assert err <= bound
            assert np.isfinite(q).all() and (q >= env.r_lo).all() and (q <= env.r_hi).all()
            assert (out["iterations"] == iters).all() and (out["start"] == 0).all()
            dist, angle = pref.pose_error(q, pos, quat, mode)
            assert np.abs(out["residual"] - dist).max() <= 2 * FK_TOL and np.abs(out["angle"] - angle).max() <= ANGLE_EVAL_TOL
    rng = np.random.default_rng(100 + n)
    targets = (np.array([15.0, -8.0, 2.0]) + np.array([7.0, 16.0, 4.0]) * rng.random((n, 3))).astype(np.float32)     # the inner box
    starts = np.random.default_rng(200 + n).uniform(-0.3, 0.3, size=(n, 6)).astype(np.float32)
    for iters in (1, 3):
        for q_init in (None, starts):
            out = solve(env, ref.POSITION, targets, None, starts=1, q_init=q_init, max_iterations=iters, tolerance=0.0)
            want, want_res, _ = ik_ref.solve_ik(targets, q_init, max_iterations=iters, tolerance=0.0)
            err = np.abs(out["q"].astype(np.float64) - want).max()
            print(f"n {n}, position, {iters} iterations, start {'rest' if q_init is None else 'given'}: joint error {err:.3g}")
            assert err <= 1e-4
            assert (out["iterations"] == iters).all() and (out["angle"] == 0).all()
            assert np.abs(out["residual"] - want_res).max() <= 1e-2
    env.close()


@pytest.mark.parametrize("n,S", SHAPES)
def test_a_start_does_not_depend_on_the_number_of_starts(n, S):
    """Start k of an S-start call (policy BEST) ends bit for bit where a one-start call from the same joints ends: all three tasks,
    a shared table and a table per env (with rows outside the limits: the clamp)."""
    from pioneer_amd import PioneerVectorEnv
    env = PioneerVectorEnv(n, device="cuda:0", seed=2)
    pos, quat = mixed_poses(n, 40 + n + S)
    box = ref.box_targets(n, 50 + S)
    rng = np.random.default_rng(60 + n + S)
    own = (rng.uniform(-1.1, 1.1, size=(n, S, 6)) * ref.LIMITS).astype(np.float32)
    keys = ("q", "residual", "angle", "iterations")
    for task in TASKS:
        p = box if task == ref.POSITION else pos
        for table in (ref.start_table(S), own):
            many = solve(env, task, p, quat, starts=table, return_all=True)
            assert many["all_q"].shape == (n, S, 6) and many["all_iterations"].shape == (n, S)
            for k in range(S):
                start = np.ascontiguousarray(np.broadcast_to(table[k], (n, 6)) if table.ndim == 2 else table[:, k])
                one = solve(env, task, p, quat, starts=1, q_init=start)
                for key in keys:
                    assert np.array_equal(many["all_" + key][:, k].view(np.uint32), one[key].view(np.uint32)), (task, table.ndim, k, key)
    env.close()


def check_selection(env, task, out, policy, q_ref):
    """Check 3 of the suite: the selection is the stated one, exactly, on the kernel's own per-start outputs."""
    n, S = out["all_iterations"].shape
    rows = np.arange(n)
    win = out["start"]
    assert ((win >= 0) & (win < S)).all()
    assert np.array_equal(out["q"].view(np.uint32), out["all_q"][rows, win].view(np.uint32))
    for key in ("residual", "angle", "iterations"):
        assert np.array_equal(out[key], out["all_" + key][rows, win])
    conv = within(task, out["all_residual"], out["all_angle"])
    its = out["all_iterations"]
    if policy == "best":
        assert np.array_equal(out["converged"], ((its < MAX_IT) | conv).sum(axis=1))
        assert (conv | (its == MAX_IT)).all()
    else:
        some = conv.any(axis=1)
        kmin = np.where(conv, its, MAX_IT + 1).min(axis=1)
        assert (its[some] == kmin[some, None]).all()                 # every start of the env stopped at the winner's check
        assert (out["iterations"][some] == kmin[some]).all()
        assert (its[~some] == MAX_IT).all()
        assert np.array_equal(out["converged"], conv.sum(axis=1))
    some = conv.any(axis=1)
    assert (conv[rows, win] == some).all()                           # the winner is converged whenever any start is
    assert ((out["converged"] > 0) == some).all()
    near = ((out["all_q"].astype(np.float64) - q_ref.astype(np.float64)[:, None]) ** 2).sum(axis=2)
    left = out["all_residual"].astype(np.float64) + (0.0 if task == ref.POSITION else WEIGHT) * out["all_angle"].astype(np.float64)
    best_near = np.where(conv, near, np.inf).min(axis=1)
    assert (near[rows, win][some] <= best_near[some] * (1 + 8 * 2.0 ** -24)).all()
    fin = ~some & np.isfinite(left).all(axis=1)                     # no start converged: the smallest error left (two roundings each)
    assert (left[rows, win][fin] <= left.min(axis=1)[fin] * (1 + 4 * 2.0 ** -24)).all()
    # among starts with the winner's cost the lowest index: the same joints (or the same error left) give the same float32 cost
    same_q = (out["all_q"].view(np.uint32) == out["q"].view(np.uint32)[:, None]).all(axis=2)
    same_left = (out["all_residual"] == out["residual"][:, None]) & (out["all_angle"] == out["angle"][:, None])
    tied = np.where(some[:, None], conv & same_q, ~conv & same_left)
    assert (tied.argmax(axis=1) == win).all()
    assert (out["q"] >= env.r_lo).all() and (out["q"] <= env.r_hi).all()
    return conv


@pytest.mark.parametrize("n,S", [(1000, 16), (64, 8), (37, 2), (37, 32), (37, 64), (1, 16)])
def test_the_selection_is_the_stated_one(n, S):
    from pioneer_amd import PioneerVectorEnv
    env = PioneerVectorEnv(n, device="cuda:0", seed=3)
    pos, quat = mixed_poses(n, 70 + S)
    box = ref.box_targets(n, 71 + S)
    rng = np.random.default_rng(72 + n + S)
    given = (rng.uniform(-0.9, 0.9, size=(n, 6)) * ref.LIMITS).astype(np.float32)
    q_init = (rng.uniform(-1.1, 1.1, size=(n, 6)) * ref.LIMITS).astype(np.float32)        # (partly outside the limits)
    table = ref.start_table(S)
    choices = 0
    for task in TASKS:
        p = box if task == ref.POSITION else pos
        for policy in ("best", "first"):
            a = solve(env, task, p, quat, starts=S, q_ref=given, policy=policy, return_all=True)
            conv = check_selection(env, task, a, policy, given)
            choices += int(((conv.sum(axis=1) > 1) & (a["start"] > 0)).sum())
            b = solve(env, task, p, quat, starts=table, policy=policy, return_all=True)                       # q_ref NULL: start 0, the rest pose
            check_selection(env, task, b, policy, np.zeros((n, 6), dtype=np.float32))
            c = solve(env, task, p, quat, starts=table, q_init=q_init, policy=policy, return_all=True)       # .. the clamped q_init
            check_selection(env, task, c, policy, np.clip(q_init, env.r_lo, env.r_hi))
            if policy == "best":                                                                              # the int S is the default table
                assert all(np.array_equal(a["all_" + k], b["all_" + k]) for k in ("q", "residual", "angle", "iterations"))
    print(f"n {n} S {S}: {choices} envs chose among several converged starts and not start 0")
    assert choices > 0 or n * S < 512
    env.close()


def test_convergence_against_the_reference():
    """The FULL set (1000 envs) at S = 16 from the default table: the GPU's share of envs with a converged start is at least the
    float64 reference's - 0.01 (a far start's float32 trajectory may end in another minimum than its float64 one), and every env
    the GPU reports converged is at the pose under the float64 chain.  The position task on the full target box at S = 8 likewise.
    Measured on an MI355X: FULL set GPU 1.000, reference 1.000 (S = 1: 0.892 both); box GPU 0.958, reference 0.958."""
    from pioneer_amd import PioneerVectorEnv
    n = ref.FULL_SET[0]
    env = PioneerVectorEnv(n, device="cuda:0", seed=4)
    pos, quat, _, per = ref.full_set_reference(16)
    want = float(per["converged_starts"].any(axis=1).mean())
    for policy in ("best", "first"):
        out = solve(env, ref.POSE, pos, quat, starts=16, policy=policy)
        ok = out["converged"] > 0
        print(f"FULL set, S = 16, {policy}: GPU share {ok.mean():.4f}, reference {want:.4f}; iterations of the winners {np.bincount(out['iterations'])}")
        assert ok.mean() >= want - 0.01
        dist, angle = pref.pose_error(out["q"], pos, quat)
        assert (dist[ok] <= TOL + 2 * FK_TOL).all() and (angle[ok] <= ANGLE_TOL + ANGLE_EVAL_TOL).all()
        assert np.abs(out["residual"] - dist)[ok].max() <= 2 * FK_TOL and np.abs(out["angle"] - angle)[ok].max() <= ANGLE_EVAL_TOL
        assert (out["q"] >= env.r_lo).all() and (out["q"] <= env.r_hi).all()
    one = solve(env, ref.POSE, pos, quat, starts=1)
    print(f"FULL set, S = 1: GPU share {(one['converged'] > 0).mean():.4f}, reference {per['converged_starts'][:, 0].mean():.4f}")
    tgt, per = ref.box_reference(8, n)
    want = float(per["converged_starts"].any(axis=1).mean())
    for policy in ("best", "first"):
        out = solve(env, ref.POSITION, tgt, None, starts=8, policy=policy)
        ok = out["converged"] > 0
        print(f"target box, S = 8, {policy}: GPU share {ok.mean():.4f}, reference {want:.4f}")
        assert ok.mean() >= want - 0.01
        dist = np.linalg.norm(tgt - ik_ref.point_position(out["q"].astype(np.float64)), axis=1)
        assert (dist[ok] <= TOL + 2 * FK_TOL).all() and np.abs(out["residual"] - dist)[ok].max() <= 2 * FK_TOL
        assert (out["q"] >= env.r_lo).all() and (out["q"] <= env.r_hi).all()
    env.close()


def test_an_envs_result_does_not_depend_on_the_batch_around_it():
    from pioneer_amd import PioneerVectorEnv
    n, S = 1000, 8
    pos, quat = mixed_poses(n, 90)
    rng = np.random.default_rng(91)
    q_ref = (rng.uniform(-0.9, 0.9, size=(n, 6)) * ref.LIMITS).astype(np.float32)
    env = PioneerVectorEnv(n, device="cuda:0", seed=2)
    one = PioneerVectorEnv(1, device="cuda:0", seed=2)
    perm = rng.permutation(n)
    for policy in ("best", "first"):
        base = solve(env, ref.POSE, pos, quat, starts=S, q_ref=q_ref, policy=policy, return_all=True)
        assert len(np.unique(base["iterations"])) >= 4 and (base["converged"] == 0).any() and (base["converged"] > 1).any()
        moved = solve(env, ref.POSE, pos[perm], quat[perm], starts=S, q_ref=q_ref[perm], policy=policy, return_all=True)
        for key in base:
            assert np.array_equal(base[key][perm].view(np.uint32), moved[key].view(np.uint32)), key
        for k in (0, 7, 8, 63, 64, 517, 999, int(np.argmax(base["converged"])), int(np.argmin(base["converged"]))):
            alone = solve(one, ref.POSE, pos[k:k + 1], quat[k:k + 1], starts=S, q_ref=q_ref[k:k + 1], policy=policy, return_all=True)
            for key in base:
                assert np.array_equal(base[key][k:k + 1].view(np.uint32), alone[key].view(np.uint32)), (k, key)
    env.close()
    one.close()


def test_bad_arguments_are_refused_and_leave_the_output_alone():
    from pioneer_amd import PioneerVectorEnv, PnrError, _lib
    n, S = 37, 8
    env = PioneerVectorEnv(n, device="cuda:0", seed=4)
    lib, h, st = env.lib, env._h, env._stream()
    fill = lambda count, dtype=torch.float32: torch.full((count,), -7, dtype=dtype, device=env.device)  # noqa: E731
    i32 = torch.int32
    outs = {"q_out": fill(n * 6 + 4), "residual_out": fill(n + 2), "angle_out": fill(n + 2), "iterations_out": fill(n + 2, i32),
            "start_out": fill(n + 2, i32), "converged_out": fill(n + 2, i32), "all_q": fill(n * S * 6 + 4), "all_residual": fill(n * S + 2),
            "all_angle": fill(n * S + 2), "all_iterations": fill(n * S + 2, i32)}
    extent = {"q_out": n * 6, "all_q": n * S * 6, "all_residual": n * S, "all_angle": n * S, "all_iterations": n * S}
    pos_np, quat_np, start_np, _ = pref.near_set(n, pref.NEAR_SEED(n))
    ins = {"target_pos": T(pos_np).cuda(), "target_quat": T(quat_np).cuda(), "starts": T(ref.start_table(S)).cuda(),
           "q_init": T(start_np).cuda(), "q_ref": torch.zeros((n, 6), device=env.device)}

    def params(base=_lib.IK_TASK_POSE, **kw):
        p = _lib.PnrIkMultiParams()
        assert lib.pnr_ik_multi_params_default(p, base) == 0
        for k, v in kw.items():
            if k in ("local_point", "local_axis"):
                for i in range(3):
                    getattr(p, k)[i] = v[i]
            else:
                setattr(p, k, v)
        return p

    def buffers(**kw):
        b = _lib.PnrIkMultiBuffers()
        b.struct_size = C.sizeof(_lib.PnrIkMultiBuffers)
        for name, t in {**ins, **outs}.items():
            setattr(b, name, t.data_ptr())
        for name, v in kw.items():
            setattr(b, name, v)
        return b

    def call(p, b=None, handle=h):
        return lib.pnr_solve_ik_multi(handle, p, buffers() if b is None else b, st)

    def refused(rc, word):
        assert rc == -1
        assert word in lib.pnr_last_error(h), lib.pnr_last_error(h)

    nan, inf = float("nan"), float("inf")
    assert call(params(), handle=None) == -1 and b"null handle" in lib.pnr_last_error(None)
    refused(lib.pnr_solve_ik_multi(h, None, buffers(), st), b"null params")
    refused(lib.pnr_solve_ik_multi(h, params(), None, st), b"null buffers")
    refused(call(params(struct_size=64)), b"params struct_size")
    refused(call(params(), buffers(struct_size=64)), b"buffers struct_size")
    refused(call(params(), buffers(q_out=None)), b"null q_out")
    for task in (_lib.IK_TASK_POSE, _lib.IK_TASK_AXIS):
        refused(call(params(task), buffers(target_quat=None)), b"null target_quat")
    for task in (-1, 3):
        refused(call(params(task=task)), b"task")
    for policy in (-1, 2):
        refused(call(params(policy=policy)), b"policy")
    for s in (0, -8, 3, 12, 65, 128):
        refused(call(params(num_starts=s)), b"num_starts")
    for s in (2, 64):
        refused(call(params(num_starts=s), buffers(starts=None)), b"null starts")
    for link in (-1, 11):
        refused(call(params(link=link)), b"link")
    for it in (0, 1025, -3):
        refused(call(params(max_iterations=it)), b"max_iterations")
    for task in (_lib.IK_TASK_POSITION, _lib.IK_TASK_POSE, _lib.IK_TASK_AXIS):
        pose = task != _lib.IK_TASK_POSITION
        for bad in (0.0, -1.0, nan, inf):
            for name in ("damping", "max_step") + (("orientation_weight",) if pose else ()):
                refused(call(params(task, **{name: bad})), name.encode())
        for bad in (-1e-9, nan, inf):
            for name in ("error_damping", "tolerance") + (("angle_tolerance",) if pose else ()):
                refused(call(params(task, **{name: bad})), b"pnr_solve_ik_multi: " + name.encode())
        refused(call(params(task, local_point=(0.0, nan, 0.0))), b"local_point")
    for axis in ((0.0, 0.0, 0.0), (0.0, inf, 0.0), (nan, 1.0, 0.0)):
        refused(call(params(_lib.IK_TASK_AXIS, local_axis=axis)), b"local_axis")
    for name, t in {**ins, **outs}.items():
        refused(call(params(), buffers(**{name: t.data_ptr() + 2})), name.encode() + b" must be")
    for name in ("q_out", "all_q"):
        refused(call(params(), buffers(**{name: outs[name].data_ptr() + 4})), name.encode() + b" must be 8-byte aligned")
    refused(call(params(), buffers(target_pos=None)), b"before the first pnr_reset")          # the env's own target before the first reset
    with pytest.raises(PnrError, match="before the first pnr_reset"):
        env.solve_ik_multi(ins["target_quat"])
    with pytest.raises(PnrError, match="local_axis"):
        env.solve_ik_multi(ins["target_quat"], ins["target_pos"], align_axis=(0.0, 0.0, 0.0))
    with pytest.raises(AssertionError, match="starts"):
        env.solve_ik_multi(ins["target_quat"], ins["target_pos"], starts=3)
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in outs.values())
    # .. and the same buffers are written by a good call (every task, both policies), nothing past the stated extents
    for task in (_lib.IK_TASK_POSITION, _lib.IK_TASK_POSE, _lib.IK_TASK_AXIS):
        for policy in (_lib.IK_MULTI_BEST, _lib.IK_MULTI_FIRST):
            for t in outs.values():
                t.fill_(-7)
            assert call(params(task, policy=policy)) == 0
            torch.cuda.synchronize()
            for name, t in outs.items():
                m = extent.get(name, n)
                assert bool((t[:m] != -7).all()) and bool((t[m:] == -7).all()), name
            assert bool((outs["converged_out"][:n] >= 1).all()) and bool((outs["residual_out"][:n] <= 1e-3).all())    # the NEAR start is start 0
    # NULL optional outputs, a NULL start and a NULL reference posture are accepted
    keep = outs["q_out"].clone()
    opt = {k: None for k in outs if k != "q_out"}
    assert call(params(_lib.IK_TASK_AXIS, policy=_lib.IK_MULTI_FIRST), buffers(**opt)) == 0
    torch.cuda.synchronize()
    assert torch.equal(outs["q_out"], keep)
    assert call(params(), buffers(q_init=None, q_ref=None, **opt)) == 0
    assert call(params(num_starts=1), buffers(q_init=None, q_ref=None, starts=None, **opt)) == 0
    assert call(params(_lib.IK_TASK_POSITION), buffers(target_quat=None, **opt)) == 0          # the position task reads no quaternion
    # a NaN target: a non-finite residual for that env only, start 0, no error, no hang
    tgt = ins["target_pos"].clone()
    tgt[5, 1] = nan
    for policy in ("best", "first"):
        for quat in (ins["target_quat"], None):
            out = env.solve_ik_multi(quat, tgt, starts=S, q_init=ins["q_init"], policy=policy)
            res, others = out["residual"].cpu().numpy(), np.arange(n) != 5
            assert not np.isfinite(res[5]) and int(out["start"][5]) == 0 and int(out["converged"][5]) == 0 and int(out["iterations"][5]) == MAX_IT
            assert np.isfinite(res[others]).all() and (res[others] <= 1e-3).all() and np.isfinite(out["q"].cpu().numpy()[others]).all()
    env.close()


def test_graph_capture_replays_the_eager_result():
    from pioneer_amd import PioneerVectorEnv
    n, S = 64, 8
    env = PioneerVectorEnv(n, device="cuda:0", seed=6)
    pos, quat, _ = pref.fk_set(n, 5)
    pos, quat = T(pos).cuda(), T(quat).cuda()
    q_ref = torch.zeros((n, 6), device=env.device)
    env.solve_ik_multi(quat, pos, starts=S)                                        # (the default table reaches the device before the capture)
    out = {k: torch.empty_like(v) for k, v in env.solve_ik_multi(quat, pos, starts=S, return_all=True).items()}
    s = torch.cuda.Stream(device=env.device)
    s.wait_stream(torch.cuda.current_stream(env.device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        env.solve_ik_multi(quat, pos, starts=S, q_ref=q_ref, return_all=True, out=out)      # warm-up on the capture stream
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            env.solve_ik_multi(quat, pos, starts=S, q_ref=q_ref, return_all=True, out=out)
    torch.cuda.synchronize()
    pos2, quat2, q2 = pref.fk_set(n, 6)
    pos.copy_(T(pos2)); quat.copy_(T(quat2)); q_ref.copy_(T(q2.astype(np.float32)))
    for t in out.values():
        t.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    eager = env.solve_ik_multi(quat, pos, starts=S, q_ref=q_ref, return_all=True)
    for k in out:
        assert torch.equal(out[k], eager[k]), k
    assert float((out["converged"] > 0).float().mean()) >= 0.9
    env.close()


def test_facade_starts():
    """starts=None is today's path, bit for bit; a full pose whose rest-pose start fails in the float64 reference (and has the most
    converged starts of the 16) is solved with starts=16."""
    from pioneer_amd import PioneerKinematicEnv, PioneerVectorEnv
    env = PioneerKinematicEnv()
    vec = PioneerVectorEnv(1, device="cuda:0", seed=0)
    target = (18.5, -3.25, 4.5)
    env.reset_world(target_position=target)
    vec.reset(target_positions=torch.tensor([target]))
    q1, r1 = env.solve_ik()
    q2, r2, _ = vec.solve_ik()
    assert np.array_equal(q1, q2[0].double().cpu().numpy()) and r1 == float(r2[0].item())
    assert env.target_reachable() == bool(vec.target_reachable()[0]) and env.target_reachable(starts=8) is True
    assert bool(vec.target_reachable(starts=8)[0]) and env.target_reachable(within=1e-3, starts=8) is True
    pos, quat, _, per = ref.full_set_reference(16)
    conv = per["converged_starts"]
    far_off = (per["all_residual"][:, 0] > 0.1) | (per["all_angle"][:, 0] > 0.1)      # (a clear failure, not a near miss of the tolerance)
    lost = np.nonzero(~conv[:, 0] & far_off & conv.any(axis=1))[0]
    k = int(lost[np.argmax(conv[lost].sum(axis=1))])
    q3, r3, a3 = env.solve_ik_pose(quat[k], target_position=pos[k])
    q4, r4, a4, _ = vec.solve_ik_pose(T(quat[k:k + 1]), T(pos[k:k + 1]))
    assert np.array_equal(q3, q4[0].double().cpu().numpy()) and r3 == float(r4[0].item()) and a3 == float(a4[0].item())
    assert r3 > TOL or a3 > ANGLE_TOL                                             # from the rest pose alone: not solved
    q5, r5, a5 = env.solve_ik_pose(quat[k], target_position=pos[k], starts=16)
    assert q5.shape == (6,) and q5.dtype == np.float64 and r5 <= TOL and a5 <= ANGLE_TOL
    dist, angle = pref.pose_error(q5[None], pos[k:k + 1], quat[k:k + 1])
    assert dist[0] <= TOL + 2 * FK_TOL and angle[0] <= ANGLE_TOL + ANGLE_EVAL_TOL
    # q_ref chooses among the solutions: the solution found nearest to another solved posture is that posture
    q6, r6, a6 = env.solve_ik_pose(quat[k], target_position=pos[k], starts=16, q_ref=q5)
    assert np.array_equal(q6, q5) and r6 == r5 and a6 == a5
    # the position task through the façade: the multi call's S = 1 is the rest-pose solve's law (error_damping 0)
    q7, r7 = env.solve_ik(target_position=(16.0, 5.0, 3.0), starts=8)
    assert r7 <= TOL and np.linalg.norm(ik_ref.point_position(q7[None])[0] - np.array([16.0, 5.0, 3.0])) <= TOL + 2 * FK_TOL
    vec.close()
    env.close()
