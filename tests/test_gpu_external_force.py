"""GPU tests of pnr_world_step_wrenches (PioneerVectorEnv.world_step(link_wrenches=...), the facade's apply_force / apply_torque)
against the float64 reference of tests/world_step_ref.py (the records: tests/external_force_ref.py), on the inputs of tests/external_force_cases.py.

Bars: the project's own for a world step re-synchronised with the float64 reference, Q_TOL / QD_TOL
(tests/bars.py).  tests/test_external_force_cpu.py asserts that on these inputs float32 rounding alone stays within a
quarter of them and that the wrenches move qd by more than ten times QD_TOL.  Every test prints its figures before it asserts.
MEASURED VALUES ON AN MI355X: see DESIGN.md 3l.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import external_force_cases as cases
import world_step_ref as wref
from bars import Q_TOL, QD_TOL
from gpu_support import bits, dev, dyn_env, dyn_words, lib as _lib, load_joints, set_motors

pytestmark = pytest.mark.gpu


def make(family, n, frame_skip=cases.FRAME_SKIP):
    """The family's env with its motors set, reset"""
    f = cases.FAMILIES[family]
    env = dyn_env(n, f["seed"], f["gravity"], frame_skip, **f["engine"])
    set_motors(env, f["motors"])
    return env


def command_r(env):
    """the env's command positions r [n, 6] (canonical state words 12..17)"""
    return env.get_state().view(torch.float32)[12:18].T.cpu().numpy()


def scenario(family, env):
    """(q, qd, wrenches, torques) of the family for this env's batch, loaded into the env"""
    q, qd = cases.states(family, command_r(env))
    load_joints(env, q, qd)
    return q, qd, cases.wrenches(family, q), cases.joint_torques(family, env.num_envs)


# ---- 6. against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(cases.FAMILIES))
@pytest.mark.parametrize("n", cases.SIZES)
def test_world_step_wrenches_against_the_reference(n, family):
    """Each family with and without joint torques, the records held for 1 sub-step, for 4 and for all: STEPS world steps, the reference
    re-synchronised with the engine before each.  At n = 1000 the reference follows every 8th env and the partial last wave."""
    f = cases.FAMILIES[family]
    env = make(family, n)
    idx = cases.followed(n)
    orc, plain = cases.make_oracle(family, len(idx), reset=False), cases.make_oracle(family, len(idx), reset=False)
    words = env.get_state().cpu().numpy().view(np.uint32)[:, idx]
    orc.load_state_words(words); plain.load_state_words(words)
    q, qd, w, tau = scenario(family, env)
    wt, tq = dev(w), dev(tau)
    worst_q = worst_qd = 0.0
    for with_tau in (False, True):
        for hold in cases.HOLDS:
            load_joints(env, q, qd)
            for step in range(cases.STEPS):
                d = dyn_words(env)[:, idx]
                orc.load_dyn_words(d)
                if step == 0 and cases.PHYS[family] & 1:
                    share = np.mean([orc.contact_wrenches(e)[0] for e in range(orc.n)])
                    print(f"family {family} n={n}: {share:.2%} of the followed envs in contact")
                    assert n < 37 or 0.05 <= share <= 0.95
                wref.world_step(orc, f["motors"], wrenches=(f["specs"], w[idx]), tau_ext=tau[idx] if with_tau else None, hold_substeps=hold)
                if step == 0:                                         # not vacuous: the wrenches matter at 10 x the bar
                    plain.load_dyn_words(d)
                    wref.world_step(plain, f["motors"], wrenches=(f["specs"], np.zeros_like(w[idx])), tau_ext=tau[idx] if with_tau else None,
                                    hold_substeps=hold)
                    effect = np.abs(orc.dstate["qd"] - plain.dstate["qd"]).max()
                    assert n < 37 or effect > 10 * QD_TOL, effect
                env.world_step(joint_torques=tq if with_tau else None, link_wrenches=(f["specs"], wt), hold_substeps=hold)
                e = dyn_words(env)[:, idx].astype(np.float64)
                dq, dqd = np.abs(e[0:6].T - orc.dstate["q"]).max(), np.abs(e[6:12].T - orc.dstate["qd"]).max()
                worst_q, worst_qd = max(worst_q, dq), max(worst_qd, dqd)
                print(f"family {family} n={n} torques={with_tau} hold={hold} step={step}: |dq| {dq:.3e} of {Q_TOL:.1e}, |dqd| {dqd:.3e} of {QD_TOL:.1e}")
                assert dq <= Q_TOL and dqd <= QD_TOL, (family, n, with_tau, hold, step, dq, dqd)
    print(f"family {family} n={n} WORST: |dq| {worst_q:.3e} |dqd| {worst_qd:.3e}")
    env.close()


# ---- 7. independent of the reference: a wrench is its joint torques ---------------------------------------------------------------
@pytest.mark.parametrize("frame", ["link", "world"])
def test_a_wrench_steps_like_its_jacobian_torques(frame):
    """frame_skip = 1: world_step(link_wrenches) == world_step(joint_torques = jacobian(link, local_point)^T [F; T]), both on the GPU,
    for a wrench on every link 1..10 (every dynamic body, body 0 included, which no contact ever loads), each sized so that it moves
    qd by many times the bar; a record on link 0 steps like no wrench at all."""
    n = 1000
    a, b, c = (make("B", n, frame_skip=1) for _ in range(3))          # the wrench, its joint torques, neither
    point = (0.5, -0.3, 0.8)                                          # in the link's frame, the same for every env
    qd = np.random.default_rng(6).uniform(-1, 1, size=(n, 6))
    zero = torch.zeros((n, 6), device="cuda:0")
    for link in range(0, 11):
        q, world, local = cases.same_wrench_both_frames(n, link, point=point, scale=cases.LINK_WRENCH_SCALE.get(link, 1.0))
        for env in (a, b, c):
            load_joints(env, q, qd)
        J = a.jacobian(link=link, local_point=point).double()
        wr = dev(world if frame == "world" else local)
        F, Tq = dev(world[:, 0, 0:3]).double(), dev(world[:, 0, 6:9]).double()   # the world force and torque
        tau = torch.einsum("nij,ni->nj", J[:, 0:3], F) + torch.einsum("nij,ni->nj", J[:, 3:6], Tq)
        a.world_step(link_wrenches=([(link, frame)], wr))
        b.world_step(joint_torques=tau.float())
        c.world_step(joint_torques=zero)
        da, db, dc = (dyn_words(e).astype(np.float64) for e in (a, b, c))
        effect = np.abs(db[6:12] - dc[6:12]).max(axis=0)
        dq, dqd = np.abs(da[0:6] - db[0:6]).max(), np.abs(da[6:12] - db[6:12]).max()
        print(f"wrench vs J^T [F; T] on the GPU, frame {frame}, link {link}: |dq| {dq:.3e} of {Q_TOL:.1e}, |dqd| {dqd:.3e} of {QD_TOL:.1e}; "
              f"the wrench moves qd by {effect.max():.3e} at most, {np.median(effect):.3e} in the median env")
        if link == 0:
            assert bool(tau.abs().max() == 0) and effect.max() == 0.0
        else:
            assert effect.max() > 10 * QD_TOL and np.median(effect) > 10 * QD_TOL
        assert dq <= Q_TOL and dqd <= QD_TOL, (link, dq, dqd)
    a.close(); b.close(); c.close()


# ---- 8. zero wrenches -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["A", "C", "Dc"])
def test_zero_wrenches_step_like_zero_torques(family):
    n = 1000
    f = cases.FAMILIES[family]
    a, b = make(family, n), make(family, n)
    q, qd, w, _ = scenario(family, a)
    load_joints(b, q, qd)
    zero_w, zero_t = torch.zeros_like(dev(w)), torch.zeros((n, 6), device="cuda:0")
    for step in range(cases.STEPS):
        b.set_dyn_state(a.get_dyn_state())
        a.world_step(joint_torques=zero_t)
        b.world_step(link_wrenches=(f["specs"], zero_w))
        da, db = dyn_words(a).astype(np.float64), dyn_words(b).astype(np.float64)
        dq, dqd = np.abs(da[0:6] - db[0:6]).max(), np.abs(da[6:12] - db[6:12]).max()
        print(f"zero wrenches family {family} step={step}: |dq| {dq:.3e} |dqd| {dqd:.3e} bit-equal {np.array_equal(da, db)}")
        assert dq <= Q_TOL and dqd <= QD_TOL
    a.close(); b.close()


# ---- 9. batch independence ----------------------------------------------------------------------------------------------------------
def test_an_env_computes_the_same_bits_whatever_the_batch():
    n, family = 1000, "C"
    f = cases.FAMILIES[family]
    env = make(family, n)
    q, qd, w, tau = scenario(family, env)
    words, d0 = env.get_state().clone(), env.get_dyn_state().clone()
    wt, tq = dev(w), dev(tau)
    for _ in range(cases.STEPS):
        env.world_step(joint_torques=tq, link_wrenches=(f["specs"], wt), hold_substeps=4)
    got = env.get_dyn_state().clone()
    assert not torch.equal(got[0:12], d0[0:12])
    for e, (m, lane) in zip([0, 1, 500, 999], [(1, 0), (64, 37), (1, 0), (70, 66)]):
        other = make(family, m)
        ws, d = other.get_state().clone(), other.get_dyn_state().clone()
        ws[:, lane], d[:, lane] = words[:, e], d0[:, e]
        other.set_state(ws); other.set_dyn_state(d)
        w2, t2 = torch.zeros((m, len(f["specs"]), 9), device="cuda:0"), torch.zeros((m, 6), device="cuda:0")
        w2[lane], t2[lane] = wt[e], tq[e]
        for _ in range(cases.STEPS):
            other.world_step(joint_torques=t2, link_wrenches=(f["specs"], w2), hold_substeps=4)
        assert torch.equal(bits(other.get_dyn_state()[:, lane]), bits(got[:, e])), e
        other.close()
    env.close()


# ---- 10. inputs and planes --------------------------------------------------------------------------------------------------------
def test_inputs_and_the_other_planes_are_left_alone():
    n, family = 100, "C"
    f = cases.FAMILIES[family]
    env = make(family, n)
    q, qd, w, tau = scenario(family, env)
    wt, tq = dev(w), dev(tau)
    w0, t0 = wt.clone(), tq.clone()
    words, d0 = env.get_state().clone(), env.get_dyn_state().clone()
    env.world_step(joint_torques=tq, link_wrenches=(f["specs"], wt))
    d1 = env.get_dyn_state()
    assert torch.equal(bits(wt), bits(w0)) and torch.equal(bits(tq), bits(t0)), "the input buffers are read only"
    assert torch.equal(bits(d1[12:36]), bits(d0[12:36])), "scales, friction and damping stay"
    assert torch.equal(bits(env.get_state()), bits(words)), "the command state stays"
    assert not torch.equal(d1[0:12], d0[0:12])
    env.close()


# ---- 11. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from pioneer_amd import EngineConfig, PioneerVectorEnv
    L = _lib()
    lib = L.load_library()
    n = 8
    P = lambda t, off=0: None if t is None else C.c_void_p(t.data_ptr() + off)  # noqa: E731
    wr = torch.ones((n * 4 * 9 + 4,), device="cuda:0")
    tq = torch.ones((n * 6 + 4,), device="cuda:0")

    def specs(*pairs):
        arr = (L.PnrLinkWrenchSpec * max(len(pairs), 1))()
        for j, (link, frame) in enumerate(pairs):
            arr[j].link, arr[j].frame = link, frame
        return arr

    def refused(h, rc, word, code=-1):
        assert rc == code, (rc, lib.pnr_last_error(h))
        assert word in lib.pnr_last_error(h), lib.pnr_last_error(h)

    good = specs((10, L.FRAME_WORLD), (3, L.FRAME_LINK))
    kin = PioneerVectorEnv(n, device="cuda:0", seed=1)
    kin.reset()
    refused(kin._h, lib.pnr_world_step_wrenches(kin._h, good, 2, P(wr), None, 0, kin._stream()), b"dynamics mode", code=-5)
    kin.close()
    env = PioneerVectorEnv(n, device="cuda:0", seed=1, engine_config=EngineConfig(mode="dynamic"))
    refused(env._h, lib.pnr_world_step_wrenches(env._h, good, 2, P(wr), None, 0, env._stream()), b"before the first pnr_reset")
    env.close()
    env = make("C", n)
    h, st = env._h, env._stream()
    before = env.get_dyn_state().clone()
    refused(h, lib.pnr_world_step_wrenches(h, None, 2, P(wr), None, 0, st), b"null specs")
    refused(h, lib.pnr_world_step_wrenches(h, good, 2, None, None, 0, st), b"null wrenches")
    refused(h, lib.pnr_world_step_wrenches(h, good, 2, P(wr, 4), None, 0, st), b"aligned")
    refused(h, lib.pnr_world_step_wrenches(h, good, 2, P(wr), P(tq, 4), 0, st), b"aligned")
    for k in (0, -1, 5, 1 << 20):
        refused(h, lib.pnr_world_step_wrenches(h, good, k, P(wr), None, 0, st), b"n_specs")
    for link in (-1, 11, 1 << 20):
        refused(h, lib.pnr_world_step_wrenches(h, specs((10, L.FRAME_WORLD), (link, L.FRAME_LINK)), 2, P(wr), None, 0, st), b"link")
    for frame in (0, 3, -1):
        refused(h, lib.pnr_world_step_wrenches(h, specs((10, frame)), 1, P(wr), None, 0, st), b"frame")
    env.set_joint_motor(2, L.CONTROL_VELOCITY_CONSTRAINT, target_velocity=0.1)
    refused(h, lib.pnr_world_step_wrenches(h, good, 2, P(wr), None, 0, st), b"constraint motor", code=-5)
    with pytest.raises(L.PnrError, match="constraint motor"):
        env.world_step(link_wrenches=([(10, "world"), ("robot:arm1", "link")], wr[:n * 18].view(n, 2, 9)))
    with pytest.raises(AssertionError):
        env.world_step(link_wrenches=([(10, "sideways")], wr[:n * 9].view(n, 1, 9)))
    with pytest.raises(AssertionError):
        env.world_step(link_wrenches=([("robot:nothing", "link")], wr[:n * 9].view(n, 1, 9)))
    with pytest.raises(AssertionError):
        env.world_step(hold_substeps=1)
    torch.cuda.synchronize()
    assert torch.equal(bits(env.get_dyn_state()), bits(before)), "a refused step leaves the state alone"
    env.set_joint_motor(2, L.CONTROL_VELOCITY, target_velocity=0.0, velocity_gain=0.0, max_force=0.0)
    assert lib.pnr_world_step_wrenches(h, good, 2, P(wr), P(tq), 1, st) == 0     # the PD law again: accepted
    env.world_step(link_wrenches=([(10, "world"), ("robot:arm1", "link")], wr[:n * 18].view(n, 2, 9)), hold_substeps=3)
    torch.cuda.synchronize()
    assert not torch.equal(env.get_dyn_state()[0:12], before[0:12])
    # device data is not inspected: a NaN record makes that env non-finite and no other
    bad = torch.zeros((n, 1, 9), device="cuda:0")
    bad[3, 0, 1] = float("nan")
    env.world_step(link_wrenches=([(10, "world")], bad))
    d = env.get_dyn_state()
    assert not bool(torch.isfinite(d[0:12, 3]).all()) and bool(torch.isfinite(d[0:12, :3]).all()) and bool(torch.isfinite(d[0:12, 4:]).all())
    env.close()


# ---- 12. graph capture ---------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_eager_result():
    n, family = 64, "C"
    f = cases.FAMILIES[family]
    env = make(family, n)
    q, qd, w, tau = scenario(family, env)
    d0 = env.get_dyn_state().clone()
    wt, tq = dev(w), dev(tau)
    s = torch.cuda.Stream(device=env.device)
    s.wait_stream(torch.cuda.current_stream(env.device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        env.world_step(joint_torques=tq, link_wrenches=(f["specs"], wt), hold_substeps=4)      # warm-up on the capture stream
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            env.world_step(joint_torques=tq, link_wrenches=(f["specs"], wt), hold_substeps=4)
    torch.cuda.synchronize()
    env.set_dyn_state(d0)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    replayed = env.get_dyn_state().clone()
    env.set_dyn_state(d0)
    env.world_step(joint_torques=tq, link_wrenches=(f["specs"], wt), hold_substeps=4)
    torch.cuda.synchronize()
    assert torch.equal(bits(replayed), bits(env.get_dyn_state()))
    assert not torch.equal(replayed[0:12], d0[0:12])
    env.close()


# ---- 13. facade -------------------------------------------------------------------------------------------------------------------------
def test_facade_apply_force_pushes_for_one_step():
    from pioneer_amd import EngineConfig, PioneerKinematicEnv
    def fresh():
        env = PioneerKinematicEnv(engine_config=EngineConfig(mode="dynamic"))
        env.reset_world(joint_positions=np.array([0.3, -0.4, 0.5, 0.2, -0.3, 0.1]), target_position=(20.0, 0.0, 4.0))
        for j in env.scene.joints:
            j.control_position(0.0, position_gain=0.0, velocity_gain=0.0)        # zero gains: no motor
        return env

    def joints(env):
        return np.array([j.position() for j in env.scene.joints] + [j.velocity() for j in env.scene.joints])

    env, still = fresh(), fresh()
    pointer = env.scene.links_by_name["robot:pointer"]
    assert env.scene.joints[5].item is env.scene.links_by_name["robot:rotator3"]
    start = joints(env)
    pointer.apply_force((0.0, 50.0, 30.0))
    env.scene.joints[3].item.apply_torque((5.0, 0.0, 0.0), frame="link")
    env.world.step(); still.world.step()
    pushed = joints(env)
    print(f"facade: the push moves qd by {np.abs(pushed[6:] - joints(still)[6:]).max():.3e}")
    assert np.abs(pushed[6:] - joints(still)[6:]).max() > 10 * QD_TOL
    assert np.array_equal(joints(still)[:6], start[:6]) and np.all(joints(still)[6:] == 0.0), "no gravity, no motor: the unpushed arm rests"
    # the next step carries no force: it equals the step of an env put into the same state and never pushed
    for j, (p, v) in zip(still.scene.joints, zip(pushed[:6], pushed[6:])):
        j.reset_state(float(p), float(v))
    assert np.array_equal(joints(still), pushed)
    env.world.step(); still.world.step()
    assert np.array_equal(joints(env), joints(still))
    # reset() drops a queued force
    pointer.apply_force((0.0, 50.0, 30.0))
    env.reset()
    assert env.world._wrenches == []
    # a fifth record raises, and the four queued before it still act
    link = env.scene.links_by_name["robot:arm2"]
    for _ in range(4):
        link.apply_force((1.0, 0.0, 0.0), position=(0.0, 0.0, 1.0), frame="link")
    with pytest.raises(AssertionError, match="at most 4"):
        link.apply_torque((0.0, 1.0, 0.0))
    env.world.step()
    assert env.world._wrenches == []
    kin = PioneerKinematicEnv()
    with pytest.raises(AssertionError, match="dynamics mode"):
        kin.scene.links_by_name["robot:pointer"].apply_force((1.0, 0.0, 0.0))
    kin.close(); still.close(); env.close()
