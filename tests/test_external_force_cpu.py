"""CPU tests of the float64 reference of pnr_world_step_wrenches (tests/world_step_ref.py's world_step on the records of
tests/external_force_ref.py) and of the inputs the GPU tests run (tests/external_force_cases.py): the reference is held against the oracle's own forward dynamics, against joint torques through
an independent Jacobian and against the oracle's world step; the inputs are shown to be well conditioned at float32 and to
matter at many times the bars.  Every test prints its figures before it asserts.
"""
import numpy as np
import pytest

import external_force_cases as cases
import external_force_ref as ref
import ik_ref
import link_kinematics_ref as lk
import oracle_cases as ocases
import world_step_ref as wref
from oracle import DynOracle

DOF = 6
Q_TOL, QD_TOL = cases.Q_TOL, cases.QD_TOL


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def random_oracle(n, seed, gravity=9.81):
    """n envs with drawn link scales at random poses and velocities"""
    orc = DynOracle(n, seed=seed, dyn=dict(gravity=gravity, randomize=1))
    orc.reset(want_obs=False)
    rng = np.random.default_rng(seed)
    lo, hi = (v.astype(np.float64) for v in ik_ref.limits_f32())
    orc.dstate["q"] = rng.uniform(0.8 * lo, 0.8 * hi, size=(n, DOF))
    orc.dstate["qd"] = rng.uniform(-2.0, 2.0, size=(n, DOF))
    return orc, rng


def test_link_table_matches_the_chain():
    """links 1-2, 3, 4, 5-6, 7, 8-10 on bodies 0..5; every link origin is its body's but the pointer's"""
    assert [ref.body_of(k) for k in range(11)] == [-1, 0, 0, 1, 2, 3, 3, 4, 5, 5, 5]
    for k in range(1, 10):
        assert np.abs(ref.link_offset(k)).max() == 0.0, k
    assert np.allclose(ref.link_offset(10), [3.6, 0.0, 1.9], rtol=0, atol=1e-15)


def test_pointer_force_matches_the_oracles_tip_force():
    n = 32
    orc, rng = random_oracle(n, 71)
    F = rng.uniform(-50, 50, size=(n, 3))
    tau = rng.uniform(-20, 20, size=(n, DOF))
    w = np.zeros((n, 1, 9))
    w[:, 0, 0:3] = F
    w[:, 0, 3:6] = ik_ref.point_position(orc.dstate["q"], 10)
    fext = ref.body_wrenches(ref.prepare([(10, "world")], w, orc.dstate["q"]), orc.dstate["q"])
    got = np.stack([orc.aba_ext(tau[e], 9.81, fext[e], e) for e in range(n)])
    want = np.stack([orc.aba(tau[e], 9.81, F[e], e) for e in range(n)])
    plain = np.stack([orc.aba(tau[e], 9.81, None, e) for e in range(n)])
    print(f"pointer force: relative difference {rel(got, want):.3e}; the force changes qdd by {np.abs(want - plain).max():.3e}")
    assert np.abs(want - plain).max() > 1.0
    assert rel(got, want) <= 1e-12


@pytest.mark.parametrize("frame", ["link", "world"])
def test_a_wrench_equals_its_joint_torques(frame):
    """aba_ext(tau, g, fext) == aba_ext(tau + J^T [F; T], g, None) with the independent float64 Jacobian of tests/ik_ref.py"""
    n = 8
    orc, rng = random_oracle(n, 72 if frame == "link" else 73)
    q = orc.dstate["q"]
    worst = 0.0
    for link in range(1, 11):
        F, P, T = rng.uniform(-30, 30, (n, 3)), rng.uniform(-1, 1, (n, 3)), rng.uniform(-15, 15, (n, 3))
        tau = rng.uniform(-20, 20, size=(n, DOF))
        R, p, _, _ = lk.link_frames(q)
        Rl = R[:, link]
        w = np.concatenate([F, P, T], axis=1)[:, None, :]
        if frame == "link":
            local, Fw, Tw = P, np.einsum("nij,nj->ni", Rl, F), np.einsum("nij,nj->ni", Rl, T)
        else:                                                         # P is a world point: its coordinates in the link's frame
            local, Fw, Tw = np.einsum("nji,nj->ni", Rl, P - p[:, link]), F, T
        fext = ref.body_wrenches(ref.prepare([(link, frame)], w, q), q)
        for e in range(n):
            J = ik_ref.jacobian(q[e:e + 1], link, local[e])[0]
            tj = J[0:3].T @ Fw[e] + J[3:6].T @ Tw[e]
            a = orc.aba_ext(tau[e], 9.81, fext[e], e)
            b = orc.aba_ext(tau[e] + tj, 9.81, None, e)
            assert np.abs(tj).max() > 0 and np.abs(a - orc.aba_ext(tau[e], 9.81, None, e)).max() > 1e-3
            worst = max(worst, rel(a, b))
    print(f"wrench == J^T [F; T], frame {frame}: worst relative difference {worst:.3e}")
    assert worst <= 1e-10


def _set_motors(orc, motors):
    """the reference's motor dictionaries on the oracle's own per-joint table"""
    for j, m in enumerate(motors):
        if m is not None:
            orc.set_joint_motor(j, m["control_mode"], m.get("target_position", 0.0), m.get("target_velocity", 0.0), m.get("position_gain"),
                                m.get("velocity_gain"), m.get("max_force"), m.get("max_velocity", 0.0))


@pytest.mark.parametrize("family", list(cases.FAMILIES))
def test_zero_wrenches_reproduce_the_oracles_world_step(family):
    n = 64
    f = cases.FAMILIES[family]
    a, b = cases.make_oracle(family, n), cases.make_oracle(family, n)
    _set_motors(b, f["motors"])
    q, qd = cases.states(family, a.state["r"])
    worst = 0.0
    for orc in (a, b):
        ocases.load_states(orc, q, qd)
    for step in range(cases.STEPS):
        wref.world_step(a, f["motors"], wrenches=(f["specs"], np.zeros((n, len(f["specs"]), 9))))
        b.world_step()
        worst = max(worst, np.abs(a.dstate["q"] - b.dstate["q"]).max(), np.abs(a.dstate["qd"] - b.dstate["qd"]).max())
    print(f"zero wrenches, family {family}: worst |reference - DynOracle.world_step| {worst:.3e}; |qd| reaches {np.abs(b.dstate['qd']).max():.3f}")
    assert np.abs(b.dstate["q"] - q).max() > 1e-3
    assert worst <= 1e-13


def test_frames_hold_and_the_welded_base():
    n = 16
    q, world, local = cases.same_wrench_both_frames(n)
    orc = cases.make_oracle("B", n)
    qd = np.random.default_rng(5).uniform(-1, 1, size=(n, DOF))

    def run(specs, w, hold, steps=1):
        orc.dstate["q"], orc.dstate["qd"] = q.copy(), qd.copy()
        first = None
        for _ in range(steps):
            out = wref.world_step(orc, cases.FREE, wrenches=(specs, w), hold_substeps=hold)
            first = out[0]["qdd"] if first is None else first
        return first, orc.dstate["qd"].copy()

    a0, _ = run([(7, "world")], world, 1)
    b0, _ = run([(7, "link")], local, 1)
    print(f"one wrench in both frames: first sub-step's qdd differs by {rel(a0, b0):.3e} (relative)")
    assert rel(a0, b0) <= 1e-12
    _, one = run([(7, "world")], world, 1)
    _, full = run([(7, "world")], world, cases.FRAME_SKIP)
    _, none = run([(7, "world")], np.zeros_like(world), 0)
    print(f"hold 1 against hold {cases.FRAME_SKIP}: qd differs by {np.abs(one - full).max():.3e} (bar {100 * QD_TOL:.1e})")
    assert np.abs(one - full).max() > 100 * QD_TOL
    _, base = run([(0, "world")], world, 0)
    _, base_l = run([(0, "link")], local, 0)
    assert np.array_equal(base, none) and np.array_equal(base_l, none), "a record on the welded base changes nothing"


def _run(family, idx, rounded, with_tau, hold, with_wrench=True, steps=cases.STEPS):
    """World steps of the reference on the envs idx of the N_MAX batch: the state after each step [steps, len(idx), 12] and the
    share of the envs in contact at the start"""
    f = cases.FAMILIES[family]
    full = cases.make_oracle(family, cases.N_MAX)
    orc = cases.make_oracle(family, len(idx), reset=False)
    orc.state[:] = full.state[idx]
    orc.dstate[:] = full.dstate[idx]
    q, qd = cases.states(family, full.state["r"], rounded)
    w = cases.wrenches(family, q, rounded)[idx].astype(np.float64)
    if not with_wrench:
        w = np.zeros_like(w)
    tau = cases.joint_torques(family, cases.N_MAX)[idx].astype(np.float64) if with_tau else None
    ocases.load_states(orc, q[idx], qd[idx])
    out = []
    share = np.mean([orc.contact_wrenches(e)[0] for e in range(orc.n)]) if cases.PHYS[family] & 1 else 0.0
    for _ in range(steps):
        wref.world_step(orc, f["motors"], wrenches=(f["specs"], w), tau_ext=tau, hold_substeps=hold)
        if rounded:
            orc.dstate["q"] = orc.dstate["q"].astype(np.float32).astype(np.float64)
            orc.dstate["qd"] = orc.dstate["qd"].astype(np.float32).astype(np.float64)
        out.append(np.concatenate([orc.dstate["q"], orc.dstate["qd"]], axis=1))
    return np.stack(out), share


FOLLOWED = np.unique(np.concatenate([np.arange(64), cases.followed(cases.N_MAX)]))


@pytest.mark.parametrize("family", list(cases.FAMILIES))
def test_the_gpu_cases_are_well_conditioned_and_the_wrenches_matter(family):
    """A condition on the chosen inputs, not a measurement of the engine: on every env a GPU test compares, rounding the inputs
    to float32 and the state to float32 after each world step moves the reference by less than a quarter of the bars, and the
    wrench changes qd after one world step by more than 10 QD_TOL — with and without joint torques, held 1 sub-step and all."""
    for with_tau in (False, True):
        for hold in cases.HOLDS:
            exact, _ = _run(family, FOLLOWED, False, with_tau, hold)
            rounded, share = _run(family, FOLLOWED, True, with_tau, hold)
            plain, _ = _run(family, FOLLOWED, True, with_tau, hold, with_wrench=False, steps=1)
            dq, dqd = np.abs(exact[:, :, 0:6] - rounded[:, :, 0:6]).max(), np.abs(exact[:, :, 6:12] - rounded[:, :, 6:12]).max()
            effect = np.abs(rounded[0, :, 6:12] - plain[0, :, 6:12]).max(axis=1)
            print(f"family {family} torques={with_tau} hold={hold}: float32 rounding moves q by {dq:.3e} (bar {Q_TOL / 4:.2e}), qd by {dqd:.3e} "
                  f"(bar {QD_TOL / 4:.1e}); the wrench changes qd by {effect.max():.3e} at most, {np.median(effect):.3e} in the median env "
                  f"(bar {10 * QD_TOL:.1e}); |qd| reaches {np.abs(rounded[:, :, 6:12]).max():.2f}")
            assert dq <= Q_TOL / 4 and dqd <= QD_TOL / 4
            assert effect.max() > 10 * QD_TOL and np.median(effect) > QD_TOL
    if cases.PHYS[family] & 1:
        print(f"family {family}: {share:.2%} of the followed envs are in contact at the start")
        assert 0.05 <= share <= 0.95
