"""pnr_world_step_targets (PioneerVectorEnv.world_step(motor_targets=..., motor_joints=...)): the world step with each env's own
motor targets for the joints of a mask — PyBullet's setJointMotorControlArray followed by stepSimulation, once per env.

The contract (include/pioneer_amd.h): env e gets what pnr_world_step gives it on a handle whose motor table holds env e's entries
as the targets of the masked joints, to float32 rounding; nothing but q, qd is written; an env's result does not depend on the
batch.  Checked per env against the float64 oracle's world step under that env's own table (PD laws), against
tests/world_step_ref.py run once per target set (constraint motors), against the engine's own pnr_world_step_torques on a
second handle (joint torques in the same launch), and bit for bit against single-env handles and eager calls (batch
independence, graph replay).  Inputs: tests/motor_target_cases.py; tests/test_motor_targets_cpu.py asserts on the oracle that
they bite.  Tolerances: the project's Q_TOL / QD_TOL for re-synchronised world steps (tests/bars.py), the engine
state loaded into the reference before every step.  Every test prints its worst deviations before it asserts.
MEASURED on an MI355X (worst |dq| rad, |dqd| rad/s over every env and step): PD laws 3.8e-7, 7.7e-6; inertia-scaled 4.1e-7, 2.7e-6;
with ground, box and link contacts 3.3e-7, 1.8e-5; the partial mask 2.8e-7, 5.9e-6; constraint motors 1.2e-7, 2.1e-6; deadbeat
|qd - v*| <= 3.6e-7 max(1, |v*|).  The 19 tests take 2.7 s.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import gpu_support
import motor_target_cases as cases
import oracle_cases as ocases
from bars import Q_TOL, QD_TOL
from gpu_support import dev, dyn_env, dyn_words, kin_env, lib as _lib, load_joints, words

pytestmark = pytest.mark.gpu

DOF = cases.DOF
NAN = float("nan")
AMPLE = 1e9                                                           # a force no sub-step here needs
INVALID, UNSUPPORTED = -1, -5


def make(n, case, engine=None, mode="dynamic", reset=True, **over):
    gravity, frame_skip = over.get("gravity", case["gravity"]), over.get("frame_skip", case["frame_skip"])
    if mode != "dynamic":
        return kin_env(n, case["seed"], reset, sim=dict(gravity=gravity, frame_skip=frame_skip), mode=mode, auto_reset=False, max_episode_steps=0)
    return dyn_env(n, case["seed"], gravity, frame_skip, reset, **(case["engine"] if engine is None else engine))


def set_motors(env, laws, tgt=None):
    """pnr_set_joint_motor for every law that is not None; tgt [12]: these targets instead of the laws' own"""
    if tgt is not None:
        laws = [m if m is None else cases.law_for_env(m, tgt, j) for j, m in enumerate(laws)]
    gpu_support.set_motors(env, laws)


def prepared(case, n, engine=None):
    """The engine and the oracle after reset, the case's command steps and its motors, held to the same command state and draws."""
    env = make(n, case, engine)
    orc = cases.make_oracle(case, n, engine)
    for act in ocases.command_actions(case["seed"], case.get("command_steps", 0), n, env.a_max):
        env.vector_step(dev(act))
    set_motors(env, case["laws"])
    w = words(env)
    assert np.array_equal(w[:21], orc.state_words()[:21]) and np.array_equal(dyn_words(env)[12:35], orc.dyn_words()[12:35])
    orc.load_state_words(w)
    return env, orc


def deviation(env, orc):
    """per env, the engine's q, qd against the oracle's: (|dq| [n], |dqd| [n])"""
    d = dyn_words(env).astype(np.float64)
    return np.abs(d[0:6].T - orc.dstate["q"]).max(axis=1), np.abs(d[6:12].T - orc.dstate["qd"]).max(axis=1)


def check(tag, env, orc):
    dq, dqd = deviation(env, orc)
    print(f"{tag}: worst |dq| {dq.max():.3e} (env {dq.argmax()}) |dqd| {dqd.max():.3e} (env {dqd.argmax()})")
    assert np.all(dq <= Q_TOL) and np.all(dqd <= QD_TOL), (tag, dq.max(), dqd.max(), np.flatnonzero((dq > Q_TOL) | (dqd > QD_TOL))[:8])


# ---- 1. PD motors against the float64 oracle, every env ---------------------------------------------------------------------
PD_SETS = [(n, e) for e in ("pd", "scaled") for n in (1, 37, 64, 1000)] + [(37, "contacts")]


@pytest.mark.parametrize("n,engine", PD_SETS)
def test_pd_motors_track_each_envs_own_targets_like_the_oracle(n, engine):
    """Full mask, per-env random targets, fresh for each of three world steps; the position law on the even joints and the
    velocity law on the odd ones; the torque law and the inertia-scaled one; one set with ground, box and link contacts."""
    c = cases.PD
    eng = {"pd": c["engine"], "scaled": cases.PD_SCALED_ENGINE, "contacts": cases.PD_CONTACT_ENGINE}[engine]
    env, orc = prepared(c, n, eng)
    for step in range(c["steps"]):
        load_joints(env, *cases.states(c, n, step))
        orc.load_dyn_words(dyn_words(env))
        tgt = cases.targets(c, n, step)
        env.world_step(motor_targets=dev(tgt))
        cases.oracle_world_step(orc, c["laws"], tgt, cases.FULL)
        check(f"targets_{engine} n={n} step={step}", env, orc)
    env.close()


# ---- 2. a partial mask next to everything else ---------------------------------------------------------------------------
def test_partial_mask_next_to_commanded_and_uncommanded_joints_and_nothing_persists():
    """Joints {0, 3, 4} masked (3 uncommanded: the handle's law on the env's targets), joint 1 commanded uniformly, joints 2 and 5
    uncommanded on a command state that vector steps moved; the unmasked joints' entries of `targets` are NaN.  The state words
    and the dyn words 12-35 are the same bits before and after the call, and the motor table is: a plain world step afterwards is
    the oracle's under the table's own targets."""
    c = cases.PARTIAL
    n, mask = c["n"], c["mask"]
    env, orc = prepared(c, n)
    st = env.state_dict()
    assert np.all(st["v"][:, [2, 5]] != 0), "the command state the unmasked, uncommanded joints track must have moved"
    for step in range(c["steps"]):
        load_joints(env, *cases.states(c, n, step))
        orc.load_dyn_words(dyn_words(env))
        tgt = cases.targets(c, n, step, mask, poison=True)
        w0, d0 = words(env), dyn_words(env)
        env.world_step(motor_targets=dev(tgt), motor_joints=mask)
        w1, d1 = words(env), dyn_words(env)
        assert np.array_equal(w0, w1), "the state words must be left bit for bit"
        assert np.array_equal(d0[12:36].view(np.uint32), d1[12:36].view(np.uint32)), "dyn words 12-35 must be left bit for bit"
        assert np.isfinite(d1[0:12]).all()
        cases.oracle_world_step(orc, c["laws"], tgt, mask)
        check(f"targets_partial step={step}", env, orc)
    load_joints(env, *cases.states(c, n, c["steps"]))
    orc.load_dyn_words(dyn_words(env))
    env.world_step()
    cases.oracle_world_step(orc, c["laws"])
    check("targets_partial, plain step afterwards", env, orc)
    env.close()


# ---- 3. constraint motors, every env, against tests/world_step_ref.py ---------------------------------------------------
@pytest.mark.parametrize("n,mask,steps", cases.CMOTOR_SETS)
def test_constraint_motors_take_each_envs_own_targets(n, mask, steps):
    """Position constraint motors with maxVelocity, velocity constraint motors (one saturating), a PD joint and an uncommanded
    joint; K = 3 target sets, each env on one of them at random; the reference runs once per set with uniform motors and each
    env is compared with the run of its own set.  The unmasked joints' entries are NaN."""
    c = cases.CMOTOR
    env, orc = prepared(c, n)
    for step in range(steps):
        q, qd = cases.states(c, n, step)
        load_joints(env, q, qd)
        orc.load_dyn_words(dyn_words(env))
        sets, pick = cases.target_sets(c, n, step, mask)
        tgt = sets[pick].copy()
        for j in range(DOF):
            if j not in mask:
                tgt[:, j] = tgt[:, DOF + j] = np.nan
        env.world_step(motor_targets=dev(tgt), motor_joints=mask)
        infos = cases.constraint_reference_step(orc, c["laws"], sets, pick, mask, c["frame_skip"])
        assert all(np.all(i["consistent"] == 1) for i in infos)
        check(f"targets_cmotor n={n} mask={mask} step={step}", env, orc)
    env.close()


# ---- 4. deadbeat, every env, with targets that are all different -----------------------------------------------------
def test_velocity_constraint_motors_are_deadbeat_on_each_envs_own_target():
    """Six velocity constraint motors with ample force, no gravity, frame_skip 1: every world step ends on the env's own v*, to
    the bound of test_velocity_motors_are_deadbeat_and_integrate_exactly."""
    L = _lib()
    c = dict(cases.PD, engine=dict(joint_damping=0.5, joint_friction=0.2))
    n = 1000
    env = make(n, c, gravity=0.0, frame_skip=1)
    load_joints(env, cases.states(c, n, 0)[0], np.zeros((n, DOF), np.float32))
    for j in range(DOF):
        env.set_joint_motor(j, L.CONTROL_VELOCITY_CONSTRAINT, target_velocity=0.0, max_force=AMPLE)
    rng = np.random.default_rng(40)
    for step in range(4):
        vs = rng.uniform(-2.0, 2.0, size=(n, DOF)).astype(np.float32)
        assert len(np.unique(vs, axis=0)) == n, "every env's targets must be its own"
        tgt = np.concatenate([np.zeros((n, DOF), np.float32), vs], axis=1)
        q0 = dyn_words(env)[0:6].T.astype(np.float64)
        env.world_step(motor_targets=dev(tgt))
        d = dyn_words(env).astype(np.float64)
        q, qd = d[0:6].T, d[6:12].T
        assert np.all((q > env.r_lo) & (q < env.r_hi)), "no joint may reach a limit here (the stop would zero its velocity)"
        err = np.abs(qd - vs) / np.maximum(1.0, np.abs(vs))
        print(f"targets_deadbeat step={step}: worst |qd - v*| / max(1, |v*|) {err.max():.3e}")
        assert np.all(err <= 1e-5), (step, err.max())
        assert np.abs(q - (q0 + vs.astype(np.float64) / 240)).max() <= 3e-7 + 1e-5 * 2.0 / 240
    env.close()


# ---- 5. with joint_torques: the engine's own pnr_world_step_torques on a second handle, set by set ---------------------
def test_joint_torques_in_the_same_launch_equal_world_step_torques_under_each_envs_table():
    c = cases.PD
    n = 64
    env, ref = make(n, c), make(n, c)
    set_motors(env, c["laws"])
    load_joints(env, *cases.states(c, n, 0))
    w0, d0 = env.get_state().clone(), env.get_dyn_state().clone()
    sets, pick = cases.target_sets(c, n, 0)
    rng = np.random.default_rng(50)
    tq = dev(rng.uniform(-500.0, 500.0, size=(n, DOF)).astype(np.float32))
    env.world_step(motor_targets=dev(sets[pick]), joint_torques=tq)
    got = dyn_words(env).astype(np.float64)
    runs = []
    for k in range(len(sets)):
        ref.set_state(w0); ref.set_dyn_state(d0)
        set_motors(ref, c["laws"], sets[k])
        ref.world_step(joint_torques=tq)
        runs.append(dyn_words(ref).astype(np.float64))
    want = np.stack(runs)[pick, :, np.arange(n)].T                  # [36, n]: env e from the run of its own set
    dq, dqd = np.abs(got[0:6] - want[0:6]).max(), np.abs(got[6:12] - want[6:12]).max()
    print(f"targets_torques: |dq| {dq:.3e} |dqd| {dqd:.3e}")
    assert dq <= Q_TOL and dqd <= QD_TOL, (dq, dqd)
    # .. and the reference's runs tell the sets apart: another set's run is off by >= 20 tolerances in at least half of the envs
    other = np.stack(runs)[(pick + 1) % len(sets), :, np.arange(n)].T
    off = np.maximum(np.abs(want[0:6] - other[0:6]).max(axis=0) / Q_TOL, np.abs(want[6:12] - other[6:12]).max(axis=0) / QD_TOL)
    assert (off >= 20.0).mean() >= 0.5, off.min()
    # the torques act: without them the result differs
    env.set_state(w0); env.set_dyn_state(d0)
    env.world_step(motor_targets=dev(sets[pick]))
    assert np.abs(dyn_words(env)[6:12] - got[6:12]).max() > 20 * QD_TOL
    env.close(); ref.close()


# ---- 6. batch independence, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["pd", "cmotor"])
def test_batch_envs_equal_single_env_handles_bit_for_bit(table):
    """Envs 0, 36, 63, 64 and 999 of an n = 1000 call equal the same envs run alone on n = 1 handles with the same calls: the PD
    table with contacts and joint torques, and the constraint table."""
    c, eng = (cases.PD, cases.PD_CONTACT_ENGINE) if table == "pd" else (cases.CMOTOR, None)
    n, steps = 1000, 3
    env = make(n, c, eng)
    set_motors(env, c["laws"])
    load_joints(env, *cases.states(c, n, 0))
    w0, d0 = env.get_state().clone(), env.get_dyn_state().clone()
    rng = np.random.default_rng(60)
    tgts = [dev(cases.targets(c, n, s)) for s in range(steps)]
    tqs = [dev(rng.uniform(-300.0, 300.0, size=(n, DOF)).astype(np.float32)) if table == "pd" else None for s in range(steps)]
    for s in range(steps):
        env.world_step(motor_targets=tgts[s], joint_torques=tqs[s])
    got = dyn_words(env)
    assert np.isfinite(got).all()
    for e in (0, 36, 63, 64, 999):
        one = make(1, c, eng)
        one.set_state(w0[:, e:e + 1].contiguous())
        one.set_dyn_state(d0[:, e:e + 1].contiguous())
        set_motors(one, c["laws"])
        for s in range(steps):
            one.world_step(motor_targets=tgts[s][e:e + 1].clone(), joint_torques=None if tqs[s] is None else tqs[s][e:e + 1].clone())
        assert np.array_equal(dyn_words(one)[:, 0].view(np.uint32), got[:, e].view(np.uint32)), e
        one.close()
    env.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_are_decided_before_any_launch_and_name_the_call():
    L = _lib()
    c = cases.PD
    n = 8
    env = make(n, c)
    set_motors(env, c["laws"])
    load_joints(env, *cases.states(c, n, 0))
    lib, st = env.lib, env._stream()
    buf = torch.zeros(n * 12 + 4, device="cuda")
    good, off4 = buf[:n * 12], buf[1:n * 12 + 1]                      # 16-byte aligned (the allocator's) and 4 bytes past it
    tq = torch.zeros(n * 6 + 4, device="cuda")
    assert good.data_ptr() % 16 == 0 and off4.data_ptr() % 16 == 4
    p = lambda t: C.c_void_p(t.data_ptr())                            # noqa: E731

    def refused(handle, code, call):
        w0 = words(handle) if handle is not None else None
        d0 = dyn_words(handle) if handle is not None and handle.engine_config.mode == "dynamic" else None
        assert call() == code
        msg = lib.pnr_last_error(handle._h if handle is not None else None)
        assert b"pnr_world_step_targets" in msg, msg
        if w0 is not None:
            assert np.array_equal(w0, words(handle))
        if d0 is not None:
            assert np.array_equal(d0.view(np.uint32), dyn_words(handle).view(np.uint32))

    refused(None, INVALID, lambda: lib.pnr_world_step_targets(None, 63, p(good), None, st))                  # a null handle
    refused(env, INVALID, lambda: lib.pnr_world_step_targets(env._h, 63, None, None, st))                    # NULL targets
    refused(env, INVALID, lambda: lib.pnr_world_step_targets(env._h, 63, p(off4), None, st))                 # misaligned targets
    refused(env, INVALID, lambda: lib.pnr_world_step_targets(env._h, 63, p(good), p(tq[1:]), st))            # misaligned joint_torques
    refused(env, INVALID, lambda: lib.pnr_world_step_targets(env._h, 0, p(good), None, st))                  # an empty mask
    refused(env, INVALID, lambda: lib.pnr_world_step_targets(env._h, 64, p(good), None, st))                 # a bit above 5
    refused(env, INVALID, lambda: lib.pnr_world_step_targets(env._h, 63 | (1 << 31), p(good), None, st))
    # a constraint motor anywhere in the table: joint torques are refused, the call without them is not
    env.set_joint_motor(2, L.CONTROL_VELOCITY_CONSTRAINT, target_velocity=0.1)
    refused(env, UNSUPPORTED, lambda: lib.pnr_world_step_targets(env._h, 63, p(good), p(tq), st))
    assert lib.pnr_world_step_targets(env._h, 63, p(good), None, st) == 0
    torch.cuda.synchronize()
    # a handle before its first pnr_reset, and a kinematic-mode handle
    fresh = make(n, c, reset=False)
    refused(fresh, INVALID, lambda: lib.pnr_world_step_targets(fresh._h, 63, p(good), None, st))
    kin = make(n, c, mode="kinematic")
    refused(kin, UNSUPPORTED, lambda: lib.pnr_world_step_targets(kin._h, 63, p(good), None, st))
    # the facade: what does not combine
    with pytest.raises(AssertionError, match="joint_state"):
        env.world_step(joint_state=torch.zeros(n, 12, device="cuda"), motor_targets=good.view(n, 12))
    with pytest.raises(AssertionError, match="link_wrenches is not built"):
        env.world_step(link_wrenches=([(10, "world")], torch.zeros(n, 1, 9, device="cuda")), motor_targets=good.view(n, 12))
    with pytest.raises(AssertionError, match="motor_joints"):
        env.world_step(motor_targets=good.view(n, 12), motor_joints=[0, 6])
    with pytest.raises(AssertionError, match="motor_joints"):
        env.world_step(motor_joints=[0])
    with pytest.raises(L.PnrError) as ei:
        env.world_step(motor_targets=good.view(n, 12), motor_joints=[])
    assert ei.value.code == INVALID
    env.close(); fresh.close(); kin.close()


# ---- 8. graph capture ----------------------------------------------------------------------------------------------------
def test_two_captured_calls_replay_with_rewritten_targets_bit_for_bit():
    """Two consecutive calls on one stream captured into a graph (one linear stream, no parallel branches), replayed after the
    targets tensor was rewritten in place: bit-equal to the eager calls with those targets."""
    c = cases.PD
    n = 1000
    env = make(n, c)
    set_motors(env, c["laws"])
    load_joints(env, *cases.states(c, n, 0))
    w0, d0 = env.get_state().clone(), env.get_dyn_state().clone()
    first, second = dev(cases.targets(c, n, 0)), dev(cases.targets(c, n, 1))
    tgt = second.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                        # eager, on the stream the capture will use
        env.world_step(motor_targets=tgt)
        env.world_step(motor_targets=tgt)
    s.synchronize()
    want = dyn_words(env)
    env.set_state(w0); env.set_dyn_state(d0)
    tgt.copy_(first)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        env.world_step(motor_targets=tgt)
        env.world_step(motor_targets=tgt)
    assert np.array_equal(dyn_words(env).view(np.uint32), d0.cpu().numpy().view(np.uint32)), "capturing must not run the calls"
    tgt.copy_(second)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    got = dyn_words(env)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(got[0:12], d0.cpu().numpy()[0:12])
    env.close()
