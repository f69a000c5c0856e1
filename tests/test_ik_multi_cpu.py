"""CPU tests of multi-start inverse kinematics (pnr_solve_ik_multi): what S starts buy in the float64 reference of
tests/ik_multi_ref.py on the set the GPU test uses, the selection's properties, the default start table, and the binding's structs."""
import ctypes as C

import numpy as np

import ik_multi_ref as ref
import ik_pose_ref as pref


def test_sixteen_starts_solve_what_one_start_does_not():
    """The FULL set (ik_pose_ref.fk_set(1000, 11): full poses of random joints at 0.8-0.9 of the limits), the default table (seed
    0), default parameters.  Measured share of envs with a converged start, float64 reference: S = 1: 0.892, 2: 0.923, 4: 0.978,
    8: 0.990, 16: 1.000.  At S = 16 an env has several converged starts, so the selection is a real choice."""
    shares = {}
    for S in (1, 2, 4, 8, 16):
        per = ref.full_set_reference(S)[3]
        shares[S] = float(per["converged_starts"].any(axis=1).mean())
    print("share of envs with a converged start:", shares)
    assert shares[16] >= 0.99
    assert shares[1] <= 0.93
    assert all(shares[a] <= shares[b] for a, b in ((1, 2), (2, 4), (4, 8), (8, 16)))      # nested tables: more starts never lose an env
    per = ref.full_set_reference(16)[3]
    assert per["converged_starts"].sum(axis=1).mean() >= 4.0


def small_problem(n=24, S=8, seed=5):
    pos, quat, _ = pref.fk_set(n, seed)
    return pos, quat, ref.start_table(S)


def test_best_takes_the_nearest_converged_start():
    pos, quat, table = small_problem()
    rng = np.random.default_rng(3)
    for q_ref in (None, rng.uniform(-0.5, 0.5, size=(len(pos), 6)) * ref.LIMITS):
        out = ref.solve_multi(ref.POSE, pos, quat, table, q_ref=q_ref)
        conv, win = out["converged_starts"], out["start"]
        want_ref = np.zeros((len(pos), 6)) if q_ref is None else q_ref
        cost = ((out["all_q"] - want_ref[:, None]) ** 2).sum(axis=2)
        assert conv.any(axis=1).sum() >= len(pos) - 2 and (conv.sum(axis=1) >= 2).any()
        for e in range(len(pos)):
            if conv[e].any():
                assert conv[e, win[e]]
                assert cost[e, win[e]] == cost[e][conv[e]].min()
                assert win[e] == np.nonzero(conv[e] & (cost[e] == cost[e, win[e]]))[0][0]
            else:
                left = out["all_residual"][e] + 10.0 * out["all_angle"][e]
                assert win[e] == int(np.argmin(left))
            assert np.array_equal(out["q"][e], out["all_q"][e, win[e]])
        assert np.array_equal(out["converged"], conv.sum(axis=1))
    # the reference posture matters: the winners differ between the two
    a = ref.solve_multi(ref.POSE, pos, quat, table)["start"]
    assert (a != win).any()


def test_first_stops_every_start_of_an_env_at_its_first_convergence():
    pos, quat, table = small_problem()
    best = ref.solve_multi(ref.POSE, pos, quat, table)
    first = ref.solve_multi(ref.POSE, pos, quat, table, policy=ref.FIRST)
    for e in range(len(pos)):
        conv = best["converged_starts"][e]
        if not conv.any():                                                          # nothing converges: FIRST is BEST
            assert first["start"][e] == best["start"][e] and np.array_equal(first["all_q"][e], best["all_q"][e])
            continue
        k = best["all_iterations"][e][conv].min()
        assert (first["all_iterations"][e] == k).all()                              # every start made exactly k iterations
        w = first["start"][e]
        assert first["converged_starts"][e, w] and best["all_iterations"][e, w] == k   # the winner is among the fastest starts
        fastest = conv & (best["all_iterations"][e] == k)
        assert np.array_equal(first["converged_starts"][e], fastest)
        assert np.array_equal(first["all_q"][e][fastest], best["all_q"][e][fastest])
        assert first["converged"][e] == fastest.sum()
    assert (first["iterations"] < best["all_iterations"].max(axis=1)).any()


def test_one_start_is_the_single_start_reference():
    pos, quat, _ = small_problem()
    start = np.random.default_rng(9).uniform(-0.3, 0.3, size=(len(pos), 6))
    want = pref.solve_ik_pose(pos, quat, start)
    for policy in (ref.BEST, ref.FIRST):
        out = ref.solve_multi(ref.POSE, pos, quat, ref.start_table(1), q_init=start, policy=policy)
        for key, w in zip(("q", "residual", "angle", "iterations"), want):
            assert np.array_equal(out[key], w)
        assert (out["start"] == 0).all()
    tgt = ref.box_targets(len(pos))
    want = ref.ik_ref.solve_ik(tgt, start)
    for policy in (ref.BEST, ref.FIRST):
        out = ref.solve_multi(ref.POSITION, tgt, None, ref.start_table(1), q_init=start, policy=policy, **ref.POSITION_DEFAULTS)
        assert np.array_equal(out["q"], want[0]) and np.array_equal(out["residual"], want[1]) and np.array_equal(out["iterations"], want[2])
        assert (out["angle"] == 0).all()


def test_a_nan_target_selects_start_zero():
    pos, quat, table = small_problem(n=5)
    pos = pos.copy()
    pos[2, 1] = np.nan
    for policy in (ref.BEST, ref.FIRST):
        out = ref.solve_multi(ref.POSE, pos, quat, table, policy=policy)
        assert out["start"][2] == 0 and not np.isfinite(out["residual"][2]) and out["converged"][2] == 0
        assert np.isfinite(np.delete(out["residual"], 2)).all()


def test_the_default_start_table():
    from pioneer_amd.scene import ik_start_table
    for S in (1, 2, 8, 64):
        t = ik_start_table(S)
        assert t.shape == (S, 6) and t.dtype == np.float32
        assert (t[0] == 0).all()
        assert (np.abs(t) <= 0.8 * ref.LIMITS.astype(np.float32) * (1 + 1e-6)).all()
        assert np.array_equal(t, ik_start_table(S, seed=0)) and np.array_equal(t, ref.start_table(S))      # reproducible; the tests' table
        assert np.array_equal(t, ik_start_table(64)[:S])                                                     # nested
        if S > 1:
            assert not np.array_equal(t, ik_start_table(S, seed=1)) and np.array_equal(ik_start_table(S, seed=1), ref.start_table(S, 1))
            assert (np.abs(t[1:]).max(axis=0) > 0.1 * ref.LIMITS).all() or S == 2


def test_binding_structs_match_the_header(hip_lib):
    from pioneer_amd import _lib
    for task, damping, err in ((_lib.IK_TASK_POSITION, 1.0, 0.0), (_lib.IK_TASK_POSE, 0.03, 0.01), (_lib.IK_TASK_AXIS, 0.03, 0.01)):
        p = _lib.PnrIkMultiParams()
        assert hip_lib.pnr_ik_multi_params_default(p, task) == 0
        assert p.struct_size == C.sizeof(_lib.PnrIkMultiParams) and p.task == task and p.policy == _lib.IK_MULTI_BEST
        assert (p.num_starts, p.starts_per_env, p.link, p.max_iterations) == (8, 0, 10, 32)
        assert (p.damping, p.error_damping, p.orientation_weight, p.max_step, p.tolerance, p.angle_tolerance) == (damping, err, 10.0, 0.5, 1e-3, 1e-3)
        assert tuple(p.local_axis) == (1.0, 0.0, 0.0) and tuple(p.local_point) == (0.0, 0.0, 0.0)
    assert hip_lib.pnr_ik_multi_params_default(_lib.PnrIkMultiParams(), 3) == -1
    assert hip_lib.pnr_ik_multi_params_default(None, 0) == -1
    assert C.sizeof(_lib.PnrIkMultiBuffers) == 8 + 15 * C.sizeof(C.c_void_p)
    # no handle: refused before anything else
    assert hip_lib.pnr_solve_ik_multi(None, _lib.PnrIkMultiParams(), _lib.PnrIkMultiBuffers(), None) == -1
