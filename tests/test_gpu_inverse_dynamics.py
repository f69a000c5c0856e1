"""GPU tests of pnr_inverse_dynamics / pnr_mass_matrix / pnr_world_step_torques (PioneerVectorEnv.inverse_dynamics, mass_matrix,
world_step(joint_torques=...) and the facade's Joint.control_torque) against the float64 reference of
tests/inverse_dynamics_ref.py (the torque step: tests/world_step_ref.py), on the inputs of tests/inverse_dynamics_cases.py.

Bars.  HARD (the project's own, tests/bars.py): a world step re-synchronised with the float64 reference agrees to
Q_TOL / QD_TOL; an acceleration error below QD_TOL / step_time = 0.048 rad/s^2 cannot move a world step outside QD_TOL, so the
engine's torques, fed to the float64 forward dynamics, must give back qdd to that, and the mass matrix must satisfy
|M_ref^-1 (M - M_ref)|_inf x 20 <= the same (20: the largest |qdd| here).  TIGHT: FLOOR_MARGIN = 8 times what float32 arithmetic
alone costs on these inputs per joint / per entry (cases.TAU_FLOOR, cases.M_FLOOR, measured on the CPU in float32 numpy;
tests/test_inverse_dynamics_cpu.py asserts them and that they are inside the hard bars).  Every test prints its figures before it
asserts.  MEASURED VALUES ON AN MI355X: see DESIGN.md 3i.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import inverse_dynamics_cases as cases
import inverse_dynamics_ref as ref
import oracle_cases as ocases
import world_step_ref as wref
from bars import Q_TOL, QD_TOL
from gpu_support import dev, dyn_env, dyn_words, f64, kin_env, lib as _lib, load_joints
from oracle import DynOracle

pytestmark = pytest.mark.gpu

HARD_ACC = QD_TOL / cases.STEP_TIME                                   # 0.048 rad/s^2
SIZES = [1, 37, 64, 1000]
SENTINEL = -7.25
TIGHT_TAU = cases.FLOOR_MARGIN * cases.TAU_FLOOR
TIGHT_M = cases.FLOOR_MARGIN * cases.M_FLOOR


def make_dyn(n, gravity=9.81, frame_skip=10, seed=cases.SEED, **eng):
    return dyn_env(n, seed, gravity, frame_skip, **eng)


def make_kin(n, gravity=9.81, reset=True, **eng):
    return kin_env(n, cases.SEED, reset, sim=dict(gravity=gravity), **eng)


def free_joints(env):
    """every joint on zero gains (the PD law): no motor torque, as one disables Bullet's default motor"""
    L = _lib()
    for j in range(6):
        env.set_joint_motor(j, L.CONTROL_VELOCITY, target_velocity=0.0, velocity_gain=0.0, max_force=0.0)


def oracle_of(env, gravity, q=None, qd=None):
    """The float64 oracle with the env's own per-env parameters (and, unless given, its simulated joints)."""
    orc = DynOracle(env.num_envs, dyn=dict(gravity=gravity))
    orc.load_dyn_words(dyn_words(env))
    if q is not None:
        ocases.load_states(orc, np.asarray(q, dtype=np.float64), np.asarray(qd, dtype=np.float64))
    return orc


# ---- 1. inverse dynamics against the reference ----------------------------------------------------------------------------------
def _source(kind, n, gravity):
    """(env, orc, joint_state tensor or None, qdd float32 [n, 6]) for a joint source"""
    q, qd, qdd = cases.joints(n)
    if kind == "kinematic_buffer":                                    # unit scales, the config's losses
        env = make_kin(n, gravity, joint_damping=0.1, joint_friction=0.1)
        orc = cases.make_oracle(n, gravity, False, joint_damping=0.1, joint_friction=0.1)
        ocases.load_states(orc, q.astype(np.float64), qd.astype(np.float64))
        assert np.all(orc.dstate["mass_scale"] == 1.0) and np.allclose(orc.dstate["damping"], 0.1, rtol=1e-7, atol=0)
        return env, orc, dev(np.concatenate([q, qd], axis=1)), qdd
    env = make_dyn(n, gravity, randomize=True)
    if kind == "dynamic_buffer":                                      # the handle's per-env scales under a caller's joints
        orc = oracle_of(env, gravity, q, qd)
        assert orc.dstate["mass_scale"].min() < 0.75 or n < 8
        return env, orc, dev(np.concatenate([q, qd], axis=1)), qdd
    assert kind == "dynamic_own"                                      # the handle's own simulated joints after two free world steps
    load_joints(env, q, qd)
    free_joints(env)
    env.world_step(); env.world_step()
    return env, oracle_of(env, gravity), None, qdd


@pytest.mark.parametrize("gravity", cases.GRAVITIES)
@pytest.mark.parametrize("kind", ["kinematic_buffer", "dynamic_buffer", "dynamic_own"])
@pytest.mark.parametrize("n", SIZES)
def test_inverse_dynamics_against_the_reference(n, kind, gravity):
    env, orc, js, qdd = _source(kind, n, gravity)
    before = None if js is None else js.clone()
    acc = dev(qdd)
    qdd64 = qdd.astype(np.float64)
    M, _, _ = ref.mass_and_bias(orc, 0.0)
    bias = {g: ref.mass_and_bias(orc, g)[2] for g in {0.0, gravity}}
    loss = wref.losses(orc)
    assert np.abs(loss).max() > 1e-3                                  # the losses flag has something to add
    for with_gravity in (True, False):
        g = gravity if with_gravity else 0.0
        for with_losses in (False, True):
            tau = f64(env.inverse_dynamics(acc, js, gravity=with_gravity, joint_losses=with_losses))
            want = np.einsum("nij,nj->ni", M, qdd64) + bias[g] + (loss if with_losses else 0.0)
            back = ref.aba(orc, tau - (loss if with_losses else 0.0), g)
            hard, tight = np.abs(back - qdd64).max(), np.abs(tau - want).max(axis=0)
            print(f"invdyn {kind} n={n} g={g} losses={with_losses}: |aba64(tau) - qdd| {hard:.3e} of {HARD_ACC:.3e}; "
                  f"|tau - ref| per joint {tight} of {TIGHT_TAU}; |tau| median {np.median(np.abs(want), axis=0)}")
            assert hard <= HARD_ACC, (kind, n, g, with_losses, hard)
            assert np.all(tight <= TIGHT_TAU), (kind, n, g, with_losses, tight / TIGHT_TAU)
    tau0 = f64(env.inverse_dynamics(None, js))                        # joint_accel=None: the bias forces
    tight0 = np.abs(tau0 - bias[gravity]).max(axis=0)
    print(f"invdyn {kind} n={n} g={gravity} accel=None: |tau - ref| per joint {tight0}")
    assert np.all(tight0 <= TIGHT_TAU), tight0 / TIGHT_TAU
    assert np.abs(ref.aba(orc, tau0, gravity)).max() <= HARD_ACC
    if js is not None:
        assert torch.equal(js, before), "the joint buffer is read only"
    # an oversized output keeps its sentinel past n * 6 floats
    big = torch.full((n * 6 + 64,), SENTINEL, dtype=torch.float32, device="cuda:0")
    rc = env.lib.pnr_inverse_dynamics(env._h, None if js is None else C.c_void_p(js.data_ptr()), C.c_void_p(acc.data_ptr()), 0,
                                      C.c_void_p(big.data_ptr()), env._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((big[n * 6:] == SENTINEL).all()) and bool((big[:n * 6] != SENTINEL).all())
    assert torch.equal(big[:n * 6].view(n, 6), env.inverse_dynamics(acc, js))
    env.close()


# ---- 2. mass matrix -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["kinematic_buffer", "dynamic_buffer", "dynamic_own"])
@pytest.mark.parametrize("n", SIZES)
def test_mass_matrix_against_the_reference(n, kind):
    env, orc, js, qdd = _source(kind, n, 9.81)
    Mref, Minv, _ = ref.mass_and_bias(orc, 0.0)
    Mt = env.mass_matrix(js)
    assert torch.equal(Mt, Mt.transpose(1, 2)), "both triangles come from one computed value"
    M = f64(Mt)
    hard = 20.0 * np.abs(np.einsum("nij,njk->nik", Minv, M - Mref)).sum(axis=2).max()
    tight = np.abs(M - Mref).max(axis=0)
    print(f"mass matrix {kind} n={n}: |Mref^-1 (M - Mref)|_inf x 20 = {hard:.3e} of {HARD_ACC:.3e}; worst entry / tight bar "
          f"{(tight / TIGHT_M).max():.3f}; diag range {np.diagonal(M, axis1=1, axis2=2).min():.3g} .. {np.diagonal(M, axis1=1, axis2=2).max():.3g}")
    assert hard <= HARD_ACC
    assert np.all(tight <= TIGHT_M), tight / TIGHT_M
    # consistency on the device alone: inverse_dynamics(qdd) - inverse_dynamics(None) = M qdd.  Two torques within TIGHT_TAU each
    # and a matrix within TIGHT_M against |qdd| <= 20: the sum of the bars
    acc = dev(qdd)
    lhs = f64(env.inverse_dynamics(acc, js)) - f64(env.inverse_dynamics(None, js))
    rhs = np.einsum("nij,nj->ni", M, qdd.astype(np.float64))
    bar = 2.0 * TIGHT_TAU + TIGHT_M @ np.full(6, 20.0)
    print(f"mass matrix {kind} n={n}: |ID(qdd) - ID(0) - M qdd| per joint {np.abs(lhs - rhs).max(axis=0)} of {bar}")
    assert np.all(np.abs(lhs - rhs).max(axis=0) <= bar)
    big = torch.full((n * 36 + 64,), SENTINEL, dtype=torch.float32, device="cuda:0")
    assert env.lib.pnr_mass_matrix(env._h, None if js is None else C.c_void_p(js.data_ptr()), C.c_void_p(big.data_ptr()), env._stream()) == 0
    torch.cuda.synchronize()
    assert bool((big[n * 36:] == SENTINEL).all()) and torch.equal(big[:n * 36].view(n, 6, 6), Mt)
    env.close()


# ---- 3. gravity hold ------------------------------------------------------------------------------------------------------------
def _hold_env(n):
    env = make_dyn(n, 9.81, seed=cases.HOLD_SEED, randomize=True, rand_friction=(0.0, 0.0), rand_damping=(0.0, 0.0))
    free_joints(env)
    load_joints(env, cases.hold_poses(n))
    return env


def test_gravity_compensation_holds_the_pose():
    """tau = inverse_dynamics() of the current state each step holds every env where it is, while the same envs fall without it.
    On the float64 reference (tests/test_inverse_dynamics_cpu.py) the smallest free-fall displacement after 24 world steps is
    0.24 rad and float32-rounded reference torques drift 2.5e-7 rad: 1 % of the fall leaves four orders to a correct kernel."""
    n, steps = 64, 24
    hold, fall = _hold_env(n), _hold_env(n)
    q0 = dyn_words(hold)[0:6].astype(np.float64)
    assert np.array_equal(q0, dyn_words(fall)[0:6].astype(np.float64))
    drift, moved = np.zeros(n), np.zeros(n)
    for _ in range(steps):
        hold.world_step(joint_torques=hold.inverse_dynamics())
        fall.world_step(joint_torques=torch.zeros((n, 6), device="cuda:0"))
        drift = np.maximum(drift, np.abs(dyn_words(hold)[0:6] - q0).max(axis=0))
        moved = np.maximum(moved, np.abs(dyn_words(fall)[0:6] - q0).max(axis=0))
    print(f"gravity hold: smallest free-fall displacement {moved.min():.4f} rad, largest hold drift {drift.max():.3e} rad")
    assert moved.min() >= 0.1, "without the torque every arm must fall"
    assert drift.max() <= 0.01 * moved.min()
    hold.close(); fall.close()


# ---- 4. computed torque ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [37, 1000])
def test_computed_torque_realises_the_acceleration(n):
    """One sub-step with tau = inverse_dynamics(qdd*, joint_losses=True): qd+ = qd + h qdd* to QD_TOL (h qdd* reaches 0.083)."""
    env = make_dyn(n, 9.81, frame_skip=1, randomize=True, rand_damping=(0.5, 0.5), rand_friction=(0.2, 0.2))
    free_joints(env)
    q, qd, qdd = cases.joints(n, frac=0.8)                            # 0.2 x the limit (>= 0.26 rad) from a limit; two sub-steps move 0.025
    load_joints(env, q, qd)
    d0 = dyn_words(env)
    assert np.all(d0[23:29] == np.float32(0.2)) and np.all(d0[29:35] == np.float32(0.5))
    tau = env.inverse_dynamics(dev(qdd), joint_losses=True)
    env.world_step(joint_torques=tau)
    got = dyn_words(env)[6:12].T.astype(np.float64)
    want = qd.astype(np.float64) + cases.H * qdd.astype(np.float64)
    err = np.abs(got - want).max()
    print(f"computed torque n={n}: |qd+ - (qd + h qdd*)| {err:.3e} of {QD_TOL:.1e}; h |qdd*| max {cases.H * np.abs(qdd).max():.3f}")
    assert cases.H * np.abs(qdd).max() > 30 * QD_TOL
    assert err <= QD_TOL
    env.close()


# ---- 5. the torque world step against the reference ---------------------------------------------------------------------------
def _torque_env(n, seed=41):
    L = _lib()
    env = make_dyn(n, 9.81, seed=seed, randomize=True, ground_z=0.0, link_contacts=True, **cases.BOX)
    for j in range(3):
        env.set_joint_motor(j, L.CONTROL_POSITION, target_position=cases.PD_TARGETS[j], target_velocity=0.0, position_gain=cases.PD_KP,
                            velocity_gain=cases.PD_KD, max_force=cases.PD_FORCES[j], max_velocity=0.0)
    for j in range(3, 6):
        env.set_joint_motor(j, L.CONTROL_VELOCITY, target_velocity=0.0, velocity_gain=0.0, max_force=0.0)
    return env


@pytest.mark.parametrize("n", SIZES)
def test_world_step_torques_against_the_reference(n):
    """Gravity, ground, box, link contacts, randomised links; joints 0-2 on PD motors whose small force caps them, joints 3-5
    free; random torques; 10 world steps, the reference re-synchronised before each.  At n = 1000 the reference (7 forward
    dynamics per env and sub-step) follows every 8th env and the whole partial last wave; the engine steps all of them."""
    env = _torque_env(n)
    q, qd, tau = cases.torque_scenario(n)
    load_joints(env, q, qd)
    law = cases.PD_KP * (np.array(cases.PD_TARGETS) - q[:, :3]) - cases.PD_KD * qd[:, :3]
    assert (np.abs(law) > np.array(cases.PD_FORCES)).mean() > 0.5, "the motors' caps must be active"
    idx = np.arange(n) if n <= 64 else np.array([e for e in range(n) if e % 8 == 0 or e >= (n // 64) * 64])
    orc, plain = cases.torque_oracle(len(idx)), cases.torque_oracle(len(idx))
    tq = dev(tau)
    worst_q = worst_qd = 0.0
    for step in range(10):
        d = dyn_words(env)[:, idx]
        orc.load_dyn_words(d)
        wref.world_step(orc, cases.TORQUE_MOTORS, tau_ext=tau[idx])
        if step == 0:                                                 # not vacuous: the torques matter at 10 x the bar
            plain.load_dyn_words(d)
            wref.world_step(plain, cases.TORQUE_MOTORS, tau_ext=np.zeros((len(idx), 6)))
            effect = np.abs(orc.dstate["qd"] - plain.dstate["qd"]).max()
            print(f"torque step n={n}: the torques change qd by {effect:.3e}")
            assert effect > 10 * QD_TOL
        env.world_step(joint_torques=tq)
        e = dyn_words(env)[:, idx].astype(np.float64)
        dq, dqd = np.abs(e[0:6].T - orc.dstate["q"]).max(), np.abs(e[6:12].T - orc.dstate["qd"]).max()
        worst_q, worst_qd = max(worst_q, dq), max(worst_qd, dqd)
        print(f"torque step n={n} step={step}: |dq| {dq:.3e} of {Q_TOL:.1e}, |dqd| {dqd:.3e} of {QD_TOL:.1e}")
        assert dq <= Q_TOL and dqd <= QD_TOL, (n, step, dq, dqd)
    env.close()


# ---- 6. zero torques ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [37, 1000])
def test_zero_torques_step_like_the_plain_world_step(n):
    a, b = _torque_env(n), _torque_env(n)
    q, qd, _ = cases.torque_scenario(n)
    load_joints(a, q, qd); load_joints(b, q, qd)
    zero = torch.zeros((n, 6), device="cuda:0")
    for step in range(5):
        b.set_dyn_state(a.get_dyn_state())
        a.world_step()
        b.world_step(joint_torques=zero)
        da, db = dyn_words(a).astype(np.float64), dyn_words(b).astype(np.float64)
        dq, dqd = np.abs(da[0:6] - db[0:6]).max(), np.abs(da[6:12] - db[6:12]).max()
        print(f"zero torques n={n} step={step}: |dq| {dq:.3e} |dqd| {dqd:.3e} bit-equal {np.array_equal(da, db)}")
        assert dq <= Q_TOL and dqd <= QD_TOL
    a.close(); b.close()


# ---- 7. batch independence ------------------------------------------------------------------------------------------------------
def test_an_env_computes_the_same_bits_whatever_the_batch():
    n = 1000
    env = _torque_env(n)
    q, qd, tau = cases.torque_scenario(n)
    _, _, qdd = cases.joints(n)
    load_joints(env, q, qd)
    words, d0 = env.get_state().clone(), env.get_dyn_state().clone()
    tq, acc = dev(tau), dev(qdd)
    idt = env.inverse_dynamics(acc, joint_losses=True).clone()
    M = env.mass_matrix().clone()
    for _ in range(3):
        env.world_step(joint_torques=tq)
    got = env.get_dyn_state().clone()
    for e, (m, lane) in zip([0, 1, 500, 999], [(1, 0), (64, 37), (1, 0), (70, 66)]):
        other = _torque_env(m)
        w, d = other.get_state().clone(), other.get_dyn_state().clone()
        w[:, lane], d[:, lane] = words[:, e], d0[:, e]
        other.set_state(w); other.set_dyn_state(d)
        t2, a2 = torch.zeros((m, 6), device="cuda:0"), torch.zeros((m, 6), device="cuda:0")
        t2[lane], a2[lane] = tq[e], acc[e]
        assert torch.equal(other.inverse_dynamics(a2, joint_losses=True)[lane], idt[e]), e
        assert torch.equal(other.mass_matrix()[lane], M[e]), e
        for _ in range(3):
            other.world_step(joint_torques=t2)
        assert torch.equal(other.get_dyn_state()[:, lane].view(torch.int32), got[:, e].view(torch.int32)), e
        other.close()
    env.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    L = _lib()
    n = 8
    lib = L.load_library()
    P = lambda t, off=0: None if t is None else C.c_void_p(t.data_ptr() + off)  # noqa: E731
    js = torch.zeros((n * 12 + 4,), device="cuda:0")
    acc = torch.zeros((n * 6 + 4,), device="cuda:0")
    tau = torch.full((n * 6 + 4,), SENTINEL, device="cuda:0")
    M = torch.full((n * 36 + 4,), SENTINEL, device="cuda:0")

    def refused(h, rc, word, code=-1):
        assert rc == code, (rc, lib.pnr_last_error(h))
        assert word in lib.pnr_last_error(h), lib.pnr_last_error(h)

    for env in (make_kin(n, reset=False), make_dyn(n)):
        h, st = env._h, env._stream()
        refused(h, lib.pnr_inverse_dynamics(h, P(js), P(acc), 0, None, st), b"null out")
        refused(h, lib.pnr_mass_matrix(h, P(js), None, st), b"null out")
        for bad in ((P(js, 4), P(acc), P(tau)), (P(js), P(acc, 4), P(tau)), (P(js), P(acc), P(tau, 4))):
            refused(h, lib.pnr_inverse_dynamics(h, bad[0], bad[1], 0, bad[2], st), b"aligned")
        refused(h, lib.pnr_mass_matrix(h, P(js, 4), P(M), st), b"aligned")
        refused(h, lib.pnr_mass_matrix(h, P(js), P(M, 4), st), b"aligned")
        for flags in (4, 7, -1, 1 << 16):
            refused(h, lib.pnr_inverse_dynamics(h, P(js), P(acc), flags, P(tau), st), b"flags")
        env_is_dyn = env.engine_config.mode == "dynamic"
        if not env_is_dyn:                                            # the handle's own joints before the first reset
            refused(h, lib.pnr_inverse_dynamics(h, None, P(acc), 0, P(tau), st), b"before the first pnr_reset")
            refused(h, lib.pnr_mass_matrix(h, None, P(M), st), b"before the first pnr_reset")
            with pytest.raises(L.PnrError, match="before the first pnr_reset"):
                env.inverse_dynamics()
            refused(h, lib.pnr_world_step_torques(h, P(acc), st), b"dynamics mode", code=-5)
        else:
            before = env.get_dyn_state().clone()
            refused(h, lib.pnr_world_step_torques(h, None, st), b"null joint_torques")
            refused(h, lib.pnr_world_step_torques(h, P(acc, 4), st), b"aligned")
            env.set_joint_motor(2, L.CONTROL_VELOCITY_CONSTRAINT, target_velocity=0.1)
            refused(h, lib.pnr_world_step_torques(h, P(acc), st), b"constraint motor", code=-5)
            with pytest.raises(L.PnrError, match="constraint motor"):
                env.world_step(joint_torques=acc[:n * 6].view(n, 6))
            assert torch.equal(env.get_dyn_state(), before), "a refused step leaves the state alone"
            env.set_joint_motor(2, L.CONTROL_VELOCITY, target_velocity=0.0, velocity_gain=0.0)
            assert lib.pnr_world_step_torques(h, P(acc), st) == 0     # the PD law again: accepted
        torch.cuda.synchronize()
        assert bool((tau == SENTINEL).all()) and bool((M == SENTINEL).all())
        assert lib.pnr_inverse_dynamics(h, P(js), P(acc), 3, P(tau), st) == 0 and lib.pnr_mass_matrix(h, P(js), P(M), st) == 0
        torch.cuda.synchronize()
        assert bool((tau[n * 6:] == SENTINEL).all()) and bool((M[n * 36:] == SENTINEL).all())
        assert bool((M[:n * 36].view(n, 6, 6).diagonal(dim1=1, dim2=2) > 0).all())
        tau.fill_(SENTINEL); M.fill_(SENTINEL)
        env.close()
    # a dynamics-mode handle has no link scales before its first reset, whatever the joint source
    from pioneer_amd import EngineConfig, PioneerVectorEnv
    env = PioneerVectorEnv(n, device="cuda:0", seed=1, engine_config=EngineConfig(mode="dynamic"))
    refused(env._h, lib.pnr_inverse_dynamics(env._h, P(js), P(acc), 0, P(tau), env._stream()), b"before the first pnr_reset")
    refused(env._h, lib.pnr_world_step_torques(env._h, P(acc), env._stream()), b"before the first pnr_reset")
    env.close()
    # non-finite input: non-finite output, no error
    env = make_kin(n)
    js2 = torch.zeros((n, 12), device="cuda:0")
    js2[0, 1] = float("nan")
    out = env.inverse_dynamics(None, js2)
    assert not bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[1:]).all())
    env.close()


# ---- 9. graph capture -----------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_eager_result():
    n = 64
    env = _torque_env(n)
    q, qd, _ = cases.torque_scenario(n)
    _, _, qdd = cases.joints(n)
    load_joints(env, q, qd)
    d0 = env.get_dyn_state().clone()
    acc = dev(0.1 * qdd)
    tau = torch.empty((n, 6), device="cuda:0")
    s = torch.cuda.Stream(device=env.device)
    s.wait_stream(torch.cuda.current_stream(env.device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        env.inverse_dynamics(acc, joint_losses=True, out=tau)        # warm-up on the capture stream
        env.world_step(joint_torques=tau)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            env.inverse_dynamics(acc, joint_losses=True, out=tau)
            env.world_step(joint_torques=tau)
    torch.cuda.synchronize()
    env.set_dyn_state(d0)
    tau.fill_(-1)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    replayed, tau_replayed = env.get_dyn_state().clone(), tau.clone()
    env.set_dyn_state(d0)
    eager_tau = env.inverse_dynamics(acc, joint_losses=True)
    env.world_step(joint_torques=eager_tau)
    torch.cuda.synchronize()
    assert torch.equal(tau_replayed, eager_tau)
    assert torch.equal(replayed.view(torch.int32), env.get_dyn_state().view(torch.int32))
    assert not torch.equal(replayed[0:12], d0[0:12])
    env.close()


# ---- 10. facade -----------------------------------------------------------------------------------------------------------------
def test_facade_control_torque_holds_the_arm_and_lasts_one_step():
    from pioneer_amd import EngineConfig, PioneerKinematicEnv, SimulationConfig
    env = PioneerKinematicEnv(simulation_config=SimulationConfig(gravity=9.81), engine_config=EngineConfig(mode="dynamic"))
    q0 = cases.hold_poses(1)[0].astype(np.float64)
    env.reset_world(joint_positions=q0, target_position=(20.0, 0.0, 4.0))
    J = env.scene.joints
    for j in J:
        j.control_position(0.0, position_gain=0.0, velocity_gain=0.0)   # zero gains: no motor
    start = np.array([j.position() for j in J])
    drift = 0.0
    for _ in range(24):
        tau = env._vec.inverse_dynamics()[0].cpu().numpy()
        for j in J:
            j.control_torque(float(tau[j.index]))
        env.world.step()
        drift = max(drift, float(np.abs(np.array([j.position() for j in J]) - start).max()))
    held = np.array([j.position() for j in J])
    for _ in range(24):                                               # no call: the torque was cleared, the arm falls
        env.world.step()
    fell = float(np.abs(np.array([j.position() for j in J]) - held).max())
    print(f"facade hold: drift {drift:.3e} rad over 24 steps, then {fell:.4f} rad of fall in 24 steps without the torque")
    assert fell >= 0.1
    assert drift <= 0.01 * fell
    kin = PioneerKinematicEnv()
    with pytest.raises(_lib().PnrError):
        kin.scene.joints[0].control_torque(1.0)
    kin.close()
    env.close()
