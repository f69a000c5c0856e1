"""The inputs of the per-env motor-target tests (tests/motor_target_cases.py) checked on the CPU with the float64 oracle: a
comparison of pnr_world_step_targets against the per-env references means something only where an env's OWN targets change its
result by far more than the tolerance.  A kernel that reads another env's row, ignores the mask or leaves the table's targets in
place must then miss the bar on most envs and on every joint.
"""
import numpy as np
import pytest

import motor_target_cases as cases
import oracle_cases as ocases

Q_TOL, QD_TOL, DOF = cases.Q_TOL, cases.QD_TOL, cases.DOF
BITE = 20.0                                                           # tolerances


def _ratio(a, b):
    """per env and joint, the difference of two oracle states in tolerances: max(|dq| / Q_TOL, |dqd| / QD_TOL)"""
    return np.maximum(np.abs(a["q"] - b["q"]) / Q_TOL, np.abs(a["qd"] - b["qd"]) / QD_TOL)


def _run(orc, case, n, step, laws, tgt, mask):
    ocases.load_states(orc, *cases.states(case, n, step))
    cases.oracle_world_step(orc, laws, tgt, mask)
    return orc.dstate.copy()


@pytest.mark.parametrize("engine", ["pd", "scaled", "contacts"])
def test_pd_inputs_bite(engine):
    """Every env's own targets against env 0's targets given to everyone: every env but env 0 differs on some joint by >= 20
    tolerances, and every joint differs by >= 20 tolerances in at least half of the envs.  (Seen: smallest per-env ratio above
    100 tolerances, per-joint shares 0.7 - 1.0.)"""
    c = cases.PD
    n = c["n"]
    eng = {"pd": c["engine"], "scaled": cases.PD_SCALED_ENGINE, "contacts": cases.PD_CONTACT_ENGINE}[engine]
    orc = cases.make_oracle(c, n, eng)
    for step in range(c["steps"]):
        tgt = cases.targets(c, n, step)
        own = _run(orc, c, n, step, c["laws"], tgt, cases.FULL)
        zero = _run(orc, c, n, step, c["laws"], np.repeat(tgt[:1], n, axis=0), cases.FULL)
        r = _ratio(own, zero)
        print(f"{engine} step {step}: smallest per-env ratio {r[1:].max(axis=1).min():.1f}, per-joint shares {(r >= BITE).mean(axis=0).round(2)}")
        assert np.all(r[0] == 0.0)
        assert np.all(r[1:].max(axis=1) >= BITE), r[1:].max(axis=1).min()
        assert np.all((r >= BITE).mean(axis=0) >= 0.5), (r >= BITE).mean(axis=0)


def test_pd_targets_differ_from_the_table():
    """.. and against the table's own targets (what a kernel that ignores `targets` computes): every env, some joint."""
    c = cases.PD
    n = c["n"]
    orc = cases.make_oracle(c, n)
    own = _run(orc, c, n, 0, c["laws"], cases.targets(c, n, 0), cases.FULL)
    table = _run(orc, c, n, 0, c["laws"], None, ())
    assert np.all(_ratio(own, table).max(axis=1) >= BITE)


def test_the_per_env_helper_without_targets_is_the_oracles_world_step():
    c = cases.PARTIAL
    n = c["n"]
    orc = cases.make_oracle(c, n)
    a = _run(orc, c, n, 0, c["laws"], None, ())
    ocases.load_states(orc, *cases.states(c, n, 0))
    orc.world_step()                                                  # the motors are orc.motors, as the helper left them
    assert np.array_equal(a["q"], orc.dstate["q"]) and np.array_equal(a["qd"], orc.dstate["qd"])


def test_partial_mask_inputs_bite_on_the_masked_joints_and_ignore_the_rest():
    """Joints 0, 3 (uncommanded: the handle's law on the env's targets) and 4 each differ by >= 20 tolerances from the unmasked
    run in at least half of the envs; the NaN entries of the unmasked joints reach nothing; the command state is put back."""
    c = cases.PARTIAL
    n, mask = c["n"], c["mask"]
    orc = cases.make_oracle(c, n)
    assert np.all(orc.state["v"][:, [2, 5]] != 0), "the command state the unmasked, uncommanded joints track must have moved"
    state0 = orc.state.copy()
    for step in range(c["steps"]):
        tgt = cases.targets(c, n, step, mask, poison=True)
        assert np.isnan(tgt[:, [1, 2, 5, 7, 8, 11]]).all() and np.isfinite(tgt[:, [0, 3, 4, 6, 9, 10]]).all()
        own = _run(orc, c, n, step, c["laws"], tgt, mask)
        assert np.isfinite(own["q"]).all() and np.isfinite(own["qd"]).all()
        assert orc.state.tobytes() == state0.tobytes()
        plain = _run(orc, c, n, step, c["laws"], None, ())
        share = (_ratio(own, plain) >= BITE).mean(axis=0)
        print(f"partial step {step}: per-joint shares {share.round(2)}")
        assert np.all(share[list(mask)] >= 0.5), share
        # a mask that forgets the uncommanded joint 3 is told apart as well
        short = _run(orc, c, n, step, c["laws"], tgt, (0, 4))
        assert (_ratio(own, short)[:, 3] >= BITE).mean() >= 0.5


@pytest.mark.parametrize("n,mask,step", [(n, mask, s) for n, mask, steps in cases.CMOTOR_SETS[:2] for s in range(steps)])
def test_constraint_target_sets_bite(n, mask, step):
    """The constraint case's K target sets: an env run under another set than its own differs by >= 20 tolerances on some
    joint, for every env and every pair of sets; every set is somebody's and no set is everybody's."""
    c = cases.CMOTOR
    orc = cases.make_oracle(c, n)
    sets, pick = cases.target_sets(c, n, step, mask)
    K = len(sets)
    assert sorted(set(pick.tolist())) == list(range(K)) and np.bincount(pick).max() < n
    ocases.load_states(orc, *cases.states(c, n, step))
    start = orc.dstate.copy()
    runs = []
    for k in range(K):
        orc.dstate[:] = start
        infos = cases.constraint_reference_step(orc, c["laws"], sets, np.full(n, k), mask, c["frame_skip"])
        assert np.all(infos[k]["consistent"] == 1)
        runs.append(orc.dstate.copy())
    for a in range(K):
        for b in range(a + 1, K):
            assert np.all(_ratio(runs[a], runs[b]).max(axis=1) >= BITE), (a, b)
    # the mixed run is each env's own set's run
    orc.dstate[:] = start
    cases.constraint_reference_step(orc, c["laws"], sets, pick, mask, c["frame_skip"])
    for k in range(K):
        assert np.array_equal(orc.dstate["qd"][pick == k], runs[k]["qd"][pick == k])
