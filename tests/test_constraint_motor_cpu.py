"""The float64 reference of the constraint motor (tests/constraint_motor_ref.py) checked on the CPU, and the conditions under
which a comparison against it means something, asserted on the input sets that tests/test_gpu_constraint_motor.py runs
(tests/constraint_motor_cases.py): the solution of the boxed problem is unique on every input, its limiting cases are the
oracle's own world step, and the inputs tell a correct solver from three wrong ones.
"""
import functools

import numpy as np
import pytest

import constraint_motor_cases as cases
import constraint_motor_ref as ref
import oracle_cases as ocases
import world_step_ref as wref
from bars import QD_TOL
from oracle import DynOracle
from oracle.binding import ORC_DEV

H = 1.0 / 240
GPU_SETS = [("mixed", 1), ("mixed", 37), ("mixed", 64), ("mixed", 1000), ("subset", 37), ("subset", 1000), ("skip10", 64), ("scaled", 64)]


@functools.lru_cache(maxsize=None)
def solved(case, n):
    """the reference's sub-step records of every step of an input set: [step][sub-step] dicts"""
    c = cases.CASES[case]
    orc = cases.make_oracle(case, n)
    out = []
    for step in range(c["steps"]):
        ocases.load_states(orc, *cases.states(case, n, step))
        out.append(wref.world_step(orc, c["motors"], frame_skip=c["frame_skip"]))
    return out


def boxed(info):
    """(A, b, rhs, F, solution) of a sub-step record, over S"""
    S = info["S"]
    return H * info["Minv"][:, S][:, :, S], info["b"][:, S], info["rhs"][:, S], info["F"], info["qd_plus"][:, S]


def test_solve_boxed_on_problems_solved_by_hand():
    A = np.array([[[2.0]]]); b = np.array([[0.0]]); rhs = np.array([[1.0]])
    tau, v, pat, margin, k, slack = ref.solve_boxed(A, b, rhs, np.array([1.0]))
    assert tau[0, 0] == 0.5 and v[0, 0] == 1.0 and pat[0, 0] == 0 and k[0] == 1 and margin[0] == 1.0      # 2 (1 - 0.5)
    tau, v, pat, margin, k, slack = ref.solve_boxed(A, b, rhs, np.array([0.25]))
    assert tau[0, 0] == 0.25 and v[0, 0] == 0.5 and pat[0, 0] == 1 and k[0] == 1 and margin[0] == 0.5
    tau, v, pat, margin, k, slack = ref.solve_boxed(A, b, -rhs, np.array([0.25]))
    assert tau[0, 0] == -0.25 and v[0, 0] == -0.5 and pat[0, 0] == -1 and k[0] == 1
    # two coupled joints, v = b + A tau with A = [[2, 1], [1, 2]], rhs = (3, 0), F = (1, 9): joint 0 clamps at +1 and its
    # torque moves joint 1 by +1, which joint 1 (free) takes back with tau_1 = -1/2: v = (2 - 1/2, 0)
    A = np.array([[[2.0, 1.0], [1.0, 2.0]]]); b = np.zeros((1, 2)); rhs = np.array([[3.0, 0.0]])
    tau, v, pat, margin, k, slack = ref.solve_boxed(A, b, rhs, np.array([1.0, 9.0]))
    assert np.allclose(tau, [[1.0, -0.5]], atol=1e-15) and np.allclose(v, [[1.5, 0.0]], atol=1e-15)
    assert pat.tolist() == [[1, 0]] and k[0] == 1 and np.allclose(slack, [[1.5, 2.0 * 8.5]], atol=1e-14) and margin[0] == slack.min()


@pytest.mark.parametrize("case,n", GPU_SETS)
def test_exactly_one_pattern_is_consistent(case, n):
    for step in solved(case, n):
        for info in step:
            assert np.all(info["consistent"] == 1), (case, n, np.bincount(info["consistent"]))
            assert info["margin"].min() >= 0
            tau, F, pat = info["tau"], info["F"], info["pattern"]
            assert np.all(np.abs(tau) <= F) and np.all(tau[pat == 1] > 0) and np.all(tau[pat == -1] < 0)


def test_ample_forces_reach_every_target():
    n = 64
    motors = [dict(m, max_force=1e9) if m and m["kind"].endswith("_constraint") else m for m in cases.CASES["subset"]["motors"]]
    orc = cases.make_oracle("subset", n)
    ocases.load_states(orc, *cases.states("subset", n, 0))
    info = wref.world_step(orc, motors, frame_skip=1)[0]
    S = info["S"]
    assert S == [0, 2, 3, 5] and np.all(info["pattern"] == 0)
    assert np.abs(info["qd_plus"][:, S] - info["rhs"][:, S]).max() <= 1e-12
    assert info["capped"][:, [0, 3]].any(0).all() and not info["capped"][:, [2, 5]].any()


CONTACTS = dict(gravity=9.81, randomize=1, ground_z=6.0, link_contacts=1, obstacle_position=(10.0, 5.0, 0.0),
                obstacle_half_extents=(0.5, 0.5, 5.0))


def _pair(n, seed):
    """two oracles on the same states: link contacts, ground, box, randomised links; q within 0.6 x the limits"""
    a, b = (DynOracle(n, seed=seed, precision=ORC_DEV, dyn=CONTACTS) for _ in range(2))
    a.reset(); b.reset()
    rng = np.random.default_rng(seed)
    q = rng.uniform(0.6 * a.r_lo.astype(np.float64), 0.6 * a.r_hi.astype(np.float64), size=(n, 6)).astype(np.float32)
    qd = rng.uniform(-1.0, 1.0, size=(n, 6)).astype(np.float32)
    for o in (a, b):
        ocases.load_states(o, q, qd)
    assert sum(a.contact_wrenches(e)[0] for e in range(n)) >= n // 4, "the scenario must have contacts"
    return a, b


def test_zero_forces_are_the_oracles_world_step_without_motors():
    n = 16
    mine, orc = _pair(n, 21)
    for j in range(6):
        orc.set_joint_motor(j, 1, target_velocity=0.0, velocity_gain=0.0)
    wref.world_step(mine, [cases.vel(0.7, 0.0)] * 6)
    orc.world_step()
    assert np.abs(mine.dstate["q"] - orc.dstate["q"]).max() <= 1e-12 and np.abs(mine.dstate["qd"] - orc.dstate["qd"]).max() <= 1e-10


@pytest.mark.parametrize("k,F,side", [(0, 50.0, 1.0), (5, 2.0, -1.0)])
def test_one_saturated_joint_is_the_oracles_constant_torque(k, F, side):
    """the scenario of test_saturated_motor_is_a_constant_torque_like_the_oracle, on both sides: the reference's integration,
    contact wrenches and torque bookkeeping against the oracle's world step (ten sub-steps, free-running)"""
    n = 16
    mine, orc = _pair(n, 22 + k)
    motors = [cases.vel(0.0, 0.0)] * 6
    motors[k] = cases.vel(side * 50.0, F)
    orc.set_joint_motor(k, 1, target_velocity=side * 1e3, velocity_gain=1e6, max_force=F)
    for j in range(6):
        if j != k:
            orc.set_joint_motor(j, 1, target_velocity=0.0, velocity_gain=0.0)
    infos = wref.world_step(mine, motors)
    orc.world_step()
    assert len(infos) == 10 and all(np.all(i["pattern"] == side) and np.all(i["tau"] == side * F) for i in infos)
    assert np.abs(mine.dstate["q"] - orc.dstate["q"]).max() <= 1e-12 and np.abs(mine.dstate["qd"] - orc.dstate["qd"]).max() <= 1e-10


def test_every_joint_is_free_and_clamped_on_either_side_in_a_share_of_the_envs():
    for step in solved("mixed", 1000):
        pat = step[0]["pattern"]
        for side in (0, 1, -1):
            share = (pat == side).mean(axis=0)
            assert np.all(share >= 0.05), (side, share)
        mixed = (pat == 0).any(axis=1) & (pat != 0).any(axis=1)
        assert mixed.mean() >= 0.5, mixed.mean()
    for step in solved("subset", 1000):
        pat = step[0]["pattern"]
        assert ((pat == 0).any(axis=1) & (pat != 0).any(axis=1)).mean() >= 0.5


def test_wrong_solvers_miss_the_solution_on_most_envs():
    """clipping the all-free torques once, a diagonal mass matrix, and an active set stopped after 2 passes each differ from
    the solution by more than 10 QD_TOL in at least half of the envs — and the same active set with 12 passes reaches it"""
    for step in solved("mixed", 1000):
        A, b, rhs, F, sol = boxed(step[0])
        wrong = dict(clip_once=cases.clip_once(A, b, rhs, F), decoupled=cases.decoupled(A, b, rhs, F),
                     two_passes=cases.active_set(A, b, rhs, F, 2)[0])
        for name, v in wrong.items():
            share = (np.abs(v - sol).max(axis=1) > 10 * QD_TOL).mean()
            assert share >= 0.5, (name, share)
        v, passes = cases.active_set(A, b, rhs, F, 12)
        assert np.abs(v - sol).max() <= 1e-12 and passes.max() < 12


@pytest.mark.parametrize("n", [37, 64, 1000])
def test_pass_counts_differ_inside_a_wave(n):
    """lanes of one 64-wide wave leave an active-set loop at different passes: at least three different counts per wave"""
    for step in solved("mixed", n):
        A, b, rhs, F, _ = boxed(step[0])
        _, passes = cases.active_set(A[:128], b[:128], rhs[:128], F, 12)
        for w in range(0, len(passes), 64):
            assert len(set(passes[w:w + 64])) >= 3, np.bincount(passes[w:w + 64])


def test_max_velocity_caps_rhs_in_a_visible_share():
    for n in (37, 1000):
        for step in solved("subset", n):
            share = step[0]["capped"][:, [0, 3]].mean(axis=0)
            assert np.all(share >= 0.2) and np.all(share <= 0.8), share


def test_the_pattern_changes_between_the_sub_steps_of_a_world_step():
    (step,) = solved("skip10", 64)
    pats = np.stack([i["pattern"] for i in step])
    assert len(step) == 10 and (pats != pats[0]).any(axis=(0, 2)).mean() >= 0.25
