"""CPU tests of the inverse-dynamics triple (pnr_inverse_dynamics, pnr_mass_matrix, pnr_world_step_torques): the float64
reference of tests/inverse_dynamics_ref.py held against independent statements, the float32 floors the GPU tests' tight bars rest
on, the conditions of the GPU scenarios asserted on the reference, and the C ABI / facade surface that needs no device.  The GPU
side is tests/test_gpu_inverse_dynamics.py."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import ik_ref
import inverse_dynamics_cases as cases
import inverse_dynamics_ref as ref
import oracle_cases as ocases
import world_step_ref as wref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch(n, gravity, randomize=True):
    q, qd, qdd = (x.astype(np.float64) for x in cases.joints(n))
    orc = cases.make_oracle(n, gravity, randomize)
    ocases.load_states(orc, q, qd)
    return orc, q, qd, qdd


def test_reference_mass_matrix_is_the_link_jacobian_sum(oracle_built):
    """M = sum over the links of s_l (Jv^T Jv + Jw^T Jw) (mass 1, inertia 1 per link, scaled), restated from the golden chain."""
    n = 64
    orc, q, _, _ = _batch(n, 9.81)
    M, Minv, _ = ref.mass_and_bias(orc, 9.81)
    sc = orc.dstate["mass_scale"]
    assert sc.min() < 0.6 and sc.max() > 1.4, "the link scales must be the drawn ones"
    Mj = np.zeros((n, 6, 6))
    for link in range(ik_ref.NUM_LINKS):
        J = ik_ref.jacobian(q, link)
        Mj += sc[:, link, None, None] * (J[:, 0:3].transpose(0, 2, 1) @ J[:, 0:3] + J[:, 3:6].transpose(0, 2, 1) @ J[:, 3:6])
    scale = np.abs(Mj).max(axis=(1, 2), keepdims=True)
    assert (np.abs(M - Mj) / scale).max() <= 1e-9
    assert (np.abs(M - M.transpose(0, 2, 1)) / scale).max() <= 1e-9
    d = np.diagonal(M, axis1=1, axis2=2)
    print("diag(M) range", d.min(), d.max())
    assert d.min() > 1.0 and d.max() > 1e3                                # light wrist, heavy base: what the bars are sized for


@pytest.mark.parametrize("gravity", cases.GRAVITIES)
def test_reference_torques_invert_the_forward_dynamics(oracle_built, gravity):
    n = 64
    orc, q, qd, qdd = _batch(n, gravity)
    tau = ref.inverse_dynamics(orc, qdd, gravity)
    err = np.abs(ref.aba(orc, tau, gravity) - qdd).max()
    print("aba(tau_ref) - qdd", err)
    assert err <= 1e-9
    # .. and the second statement (world-frame Newton-Euler over the URDF links) gives the same torques
    ne = ref.newton_euler(q, qd, qdd, orc.dstate["mass_scale"], gravity)
    assert np.abs(ne - tau).max() <= 1e-9 * np.abs(tau).max()
    bias = ref.inverse_dynamics(orc, None, gravity)
    assert np.abs(ref.newton_euler(q, qd, 0 * qdd, orc.dstate["mass_scale"], gravity) - bias).max() <= 1e-9 * np.abs(tau).max()
    # the losses are the sub-step's own terms: with them the engine's free dynamics realise qdd
    orc.d.gravity = gravity
    qdd_free, Minv = wref.free_dynamics(orc, cases.FREE_MOTORS)
    tl = ref.inverse_dynamics(orc, qdd, gravity, joint_losses=True)
    # (1e-8: free_dynamics takes M^-1 from differences of accelerations of the size of qdd_free, which costs it a digit)
    assert np.abs(qdd_free + np.einsum("nij,nj->ni", Minv, tl) - qdd).max() <= 1e-8
    # .. and so does the torque step's own path, the forward dynamics of losses + tau_ext directly (no difference: 1e-9)
    direct = np.abs(wref.accelerations(orc, cases.FREE_MOTORS, tau_ext=tl) - qdd).max()
    print("accelerations(tau_ext) - qdd", direct)
    assert direct <= 1e-9
    assert np.abs(tl - tau).max() > 0.05                                  # the drawn friction and damping do something


def test_float32_floor_constants_hold_on_the_inputs(oracle_built):
    """TAU_FLOOR / M_FLOOR are what float32 costs on the GPU tests' inputs (floor <= constant <= 2 floor, the slack for another
    libm), and each torque constant is at most 1e-4 of the batch's median |tau_i|: else the inputs are wrong, not the bound."""
    n = cases.N_MAX
    q, qd, qdd = cases.joints(n)
    ones = np.ones((n, 11))
    orc = cases.make_oracle(n, 9.81, True)
    sc, fr, da = (orc.dstate[k].copy() for k in ("mass_scale", "friction", "damping"))
    ocases.load_states(orc, q, qd)
    cases.free_joints(orc)
    orc.world_step(); orc.world_step()                                    # the "own simulated joints" source of the GPU test
    qs, qds = orc.dstate["q"].astype(np.float32), orc.dstate["qd"].astype(np.float32)
    worst = np.zeros(6)
    for g in cases.GRAVITIES:
        for qq, qqd, s in ((q, qd, ones), (q, qd, sc), (qs, qds, sc)):
            for acc in (qdd, np.zeros_like(qdd)):
                for loss in (False, True):
                    f, med = cases.tau_floor(qq, qqd, acc, s, g, fr if loss else None, da if loss else None)
                    worst = np.maximum(worst, f)
                    assert np.all(cases.TAU_FLOOR <= 1e-4 * med), (g, loss, cases.TAU_FLOOR / med)
    print("float32 floor of tau per joint", worst)
    assert np.all(worst <= cases.TAU_FLOOR) and np.all(cases.TAU_FLOOR <= 2 * worst), worst
    mf = np.max([cases.m_floor(qq, s) for qq, s in ((q, ones), (q, sc), (qs, sc))], axis=0)
    mf = np.maximum(mf, mf.T)
    print("float32 floor of M per entry\n", mf)
    assert np.array_equal(cases.M_FLOOR, cases.M_FLOOR.T)
    assert np.all(mf <= cases.M_FLOOR) and np.all(cases.M_FLOOR <= 2 * mf), mf


def test_tight_bars_are_inside_the_hard_bars(oracle_built):
    """A torque off by the whole tight bar moves the forward dynamics by less than QD_TOL / step_time, and a mass matrix off by
    its tight bar passes the hard bar on M: the tight bars are the stricter ones."""
    n = 256
    orc, q, qd, qdd = _batch(n, 9.81)
    M, Minv, _ = ref.mass_and_bias(orc, 9.81)
    hard = 2e-3 / cases.STEP_TIME
    worst = np.abs(Minv) @ (cases.FLOOR_MARGIN * cases.TAU_FLOOR)
    print("|M^-1| (8 TAU_FLOOR)", worst.max(), "of", hard)
    assert worst.max() <= hard
    dm = np.abs(Minv) @ (cases.FLOOR_MARGIN * cases.M_FLOOR)
    assert 20.0 * dm.sum(axis=2).max() <= hard


def test_gravity_hold_scenario_on_the_reference(oracle_built):
    """The scenario of the GPU gravity-hold test on the float64 reference: the smallest free-fall displacement over the batch
    after 24 world steps, and the drift of a hold with float32-rounded reference torques, which must be far below 1 % of it."""
    n = 64
    fall, hold = hold_scenario(n)
    print("smallest free-fall displacement", fall.min(), "largest float32-torque hold drift", hold.max())
    assert fall.min() >= 0.1
    assert hold.max() <= 0.1 * 0.01 * fall.min()


def hold_scenario(n, steps=24):
    q0 = cases.hold_poses(n).astype(np.float64)
    out = []
    for held in (False, True):
        orc = cases.make_oracle(n, 9.81, True, seed=cases.HOLD_SEED)
        orc.dstate["friction"] = 0.0
        orc.dstate["damping"] = 0.0
        ocases.load_states(orc, q0, np.zeros_like(q0))
        drift = np.zeros(n)
        for _ in range(steps):
            tau = ref.inverse_dynamics(orc, None, 9.81).astype(np.float32).astype(np.float64) if held else np.zeros((n, 6))
            wref.world_step(orc, cases.FREE_MOTORS, tau_ext=tau)
            drift = np.maximum(drift, np.abs(orc.dstate["q"] - q0).max(axis=1))
        out.append(drift)
    return out[0], out[1]


# ---- the ABI surface that needs no device ---------------------------------------------------------------------------------------
def test_the_three_entry_points_exist_and_refuse_a_null_handle(hip_lib):
    out = (C.c_float * 64)()
    P = lambda a: C.cast(a, C.c_void_p)  # noqa: E731
    assert hip_lib.pnr_inverse_dynamics(None, None, None, 0, P(out), None) == -1
    assert hip_lib.pnr_mass_matrix(None, None, P(out), None) == -1
    assert hip_lib.pnr_world_step_torques(None, P(out), None) == -1
    assert hip_lib.pnr_abi_version() == 5
    assert all(v == 0.0 for v in out)


def test_flag_constants_are_the_headers():
    from pioneer_amd import _lib
    with open(os.path.join(ROOT, "include", "pioneer_amd.h")) as f:
        text = f.read()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+PNR_INVDYN_(\w+)\s+(\d+)", text, re.M)}
    assert vals == {"NO_GRAVITY": _lib.INVDYN_NO_GRAVITY, "JOINT_LOSSES": _lib.INVDYN_JOINT_LOSSES} == {"NO_GRAVITY": 1, "JOINT_LOSSES": 2}
    for name in ("pnr_inverse_dynamics", "pnr_mass_matrix", "pnr_world_step_torques"):
        assert name in _lib.SIGNATURES and re.search(r"^int %s\(" % name, text, re.M), name


def test_control_torque_raises_without_a_simulated_arm():
    """Joint.control_torque on a kinematic-mode env, and next to the constraint motors, raises what the other control_* methods
    raise there (a PnrError) and records nothing.  The env is a stand-in: no engine handle is needed to refuse."""
    from pioneer_amd import _lib, model
    from pioneer_amd.scene import Joint, World

    def stand_in(mode, joint_motor):
        env = types.SimpleNamespace()
        env._vec = types.SimpleNamespace(engine_config=types.SimpleNamespace(mode=mode, joint_motor=joint_motor))
        env.joint_limits = lambda: (-np.ones(6, dtype=np.float32), np.ones(6, dtype=np.float32))
        env.simulation_config = types.SimpleNamespace(timestep=1.0 / 240, frame_skip=10, gravity=9.81)
        env.world = World(env)
        return env, Joint(env, 2, model.revolute_joints()[2])

    for mode, motor in (("kinematic", "pd"), ("dynamic", "constraint")):
        env, joint = stand_in(mode, motor)
        with pytest.raises(_lib.PnrError):
            joint.control_torque(1.5)
        assert env.world._torques == {}
    env, joint = stand_in("dynamic", "pd")
    joint.control_torque(1.5)
    assert env.world._torques == {2: 1.5}
