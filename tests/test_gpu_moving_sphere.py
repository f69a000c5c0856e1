"""GPU tests of the moving sphere (pnr_set_body_params / pnr_set_body_state / pnr_get_body_state and the world step's kWorldBody
forms; PioneerVectorEnv.set_body, the facade's create_body_sphere(mass > 0)) against the float64 reference of
tests/world_step_ref.py (the sphere's law: tests/moving_sphere_ref.py), on the inputs of tests/moving_sphere_cases.py.

Bars.  Joints: Q_TOL / QD_TOL (tests/bars.py), the project's bars for a world step re-synchronised with the float64 reference.
Sphere: 4 x the reference's own float32-storage deviation on the same inputs (cases.sphere_bars; the ratio the CPU tests hold the
joint bars to), the position bar capped at PTR_TOL.  tests/test_moving_sphere_cpu.py asserts the conditions on the inputs.  Every
test prints its figures before it asserts.
MEASURED ON AN MI355X (worst over both sizes, the three call forms and three world steps; DESIGN.md 3q has the table):
    family A  joints |dq| 7.8e-7 |dqd| 1.8e-5; sphere |dx| 9.5e-6 of 3.7e-5, |dv| 1.9e-4 of 9.4e-4
    family B  joints |dq| 6.7e-7 |dqd| 2.7e-5; sphere |dx| 9.5e-6 of 3.7e-5, |dv| 1.3e-4 of 4.5e-4
    family C  joints |dq| 6.7e-7 |dqd| 1.4e-5; sphere |dx| 1.2e-5 of 3.6e-5, |dv| 1.6e-4 of 6.5e-4
    the sphere's push against J^T (-F): |dq| 6.0e-8 |dqd| 9.8e-7; rest: |dz| 4.5e-8, |v| 1.8e-6; envs with mass <= 0: joints bit-equal
"""
import ctypes as C

import numpy as np
import pytest
import torch

import moving_sphere_cases as cases
import moving_sphere_ref as ref
import world_step_ref as wref
from bars import Q_TOL, QD_TOL
from gpu_support import bits, dev, dyn_words, engine_config_from_oracle_names, kin_env, lib as _lib, load_joints

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
H = cases.H


def make(family, n, frame_skip=cases.FRAME_SKIP, sphere=True, **dyn):
    """the family's env, reset, with the sphere enabled (every env inert until a state is set)"""
    from pioneer_amd import PioneerVectorEnv, SimulationConfig
    f = cases.FAMILIES[family]
    env = PioneerVectorEnv(n, device="cuda:0", seed=f["seed"], simulation_config=SimulationConfig(gravity=f["gravity"], frame_skip=frame_skip),
                           engine_config=engine_config_from_oracle_names(dict(f["dyn"], **dyn), auto_reset=False, max_episode_steps=0))
    env.reset()
    if sphere:
        env.set_body()
    return env


def command_r(env):
    return env.get_state().view(torch.float32)[12:18].T.cpu().numpy()


def body_words(env):
    """[8, N] float32 on the host"""
    return env.body_state().T.cpu().numpy()


def call(env, form, tq, tg):
    if form == "plain":
        env.world_step()
    elif form == "torques":
        env.world_step(joint_torques=tq)
    else:
        env.world_step(joint_torques=tq, motor_targets=tg, motor_joints=cases.TARGET_JOINTS)


# ---- 1. against the reference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", cases.FORMS)
@pytest.mark.parametrize("family", list(cases.FAMILIES))
@pytest.mark.parametrize("n", cases.SIZES)
def test_world_step_with_a_sphere_against_the_reference(n, family, form):
    """STEPS world steps, the reference re-synchronised with the engine before each.  At n = 1000 the reference follows every 8th
    env and the partial last wave."""
    env = make(family, n)
    idx = cases.followed(n)
    orc = cases.make_oracle(family, len(idx), reset=False)
    orc.load_state_words(env.get_state().cpu().numpy().view(np.uint32)[:, idx])
    r = command_r(env)
    q, qd = cases.states(family, r)
    load_joints(env, q, qd)
    w0 = cases.spheres(family, q)
    env.set_body_state(dev(w0.T))
    tau, tg = cases.joint_torques(family, n), cases.targets(family, r)
    tq, tgd = dev(tau), dev(tg)
    te, tt, joints = cases.form_inputs(form, tau[idx], tg[idx])
    bar_x, bar_v = cases.sphere_bars(family)
    worst = dict(q=0.0, qd=0.0, x=0.0, v=0.0)
    for step in range(cases.STEPS):
        orc.load_dyn_words(dyn_words(env)[:, idx])
        before = body_words(env)
        s = ref.from_words(before[:, idx])
        first = wref.world_step(orc, cases.TRACK, sphere=s, tau_ext=te, targets=tt, joints=joints)[0]
        on_arm, on_static = first["on_arm"], first["on_static"]
        live = s["m"] > 0
        if step == 0:
            print(f"family {family} n={n} {form}: {on_arm.mean():.2%} of the followed envs' spheres touch the arm, "
                  f"{on_static[live].mean():.2%} the static world; {1 - live.mean():.2%} have none")
        call(env, form, tq, tgd)
        e = dyn_words(env)[:, idx].astype(np.float64)
        after = body_words(env)
        got = ref.from_words(after[:, idx])
        dq, dqd = np.abs(e[0:6].T - orc.dstate["q"]).max(), np.abs(e[6:12].T - orc.dstate["qd"]).max()
        dx, dv = np.abs(got["x"] - s["x"])[live].max(), np.abs(got["v"] - s["v"])[live].max()
        for k, v in dict(q=dq, qd=dqd, x=dx, v=dv).items():
            worst[k] = max(worst[k], float(v))
        print(f"family {family} n={n} {form} step={step}: |dq| {dq:.3e} of {Q_TOL:.1e}, |dqd| {dqd:.3e} of {QD_TOL:.1e}, "
              f"sphere |dx| {dx:.3e} of {bar_x:.3e}, |dv| {dv:.3e} of {bar_v:.3e}")
        gone = before[6] <= 0                                          # every env of the batch, followed or not
        assert np.array_equal(after[:, gone].view(np.uint32), before[:, gone].view(np.uint32)), "an env without a sphere had its words written"
        assert np.array_equal(after[6:8].view(np.uint32), before[6:8].view(np.uint32)), "mass and radius are never written"
        assert dq <= Q_TOL and dqd <= QD_TOL, (family, n, form, step, dq, dqd)
        assert dx <= bar_x and dv <= bar_v, (family, n, form, step, dx, bar_x, dv, bar_v)
    print(f"family {family} n={n} {form} WORST: |dq| {worst['q']:.3e} |dqd| {worst['qd']:.3e} sphere |dx| {worst['x']:.3e} |dv| {worst['v']:.3e}")
    env.close()


# ---- 2. independent of the reference: the sphere's push is its Jacobian torques -----------------------------------------------------
def test_the_arm_steps_as_under_the_reaction_read_back_from_the_sphere():
    """frame_skip 1, gravity 0, no static bodies, the sphere overlapping the pointer: F = m dv / h read back from the sphere is the
    pointer's force on it, and the arm's step equals world_step(joint_torques = J_pointer(tip)^T (-F)) on a twin env."""
    from pioneer_amd import EngineConfig, PioneerVectorEnv, SimulationConfig
    n = 97
    a, b, c = (PioneerVectorEnv(n, device="cuda:0", seed=81, simulation_config=SimulationConfig(gravity=0.0, frame_skip=1),
                                engine_config=EngineConfig(mode="dynamic", auto_reset=False, max_episode_steps=0)) for _ in range(3))
    for env in (a, b, c):
        env.reset()
    q = command_r(a)                                                   # at the command state, at rest: the motors do not pull
    for env in (a, b, c):
        load_joints(env, q, None)
    rng = np.random.default_rng(82)
    tip, rad = cases.sample_positions(q, 0)
    m, r = rng.uniform(0.5, 4.0, n), rng.uniform(0.3, 1.5, n)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    x = tip[:, 0] + (rng.uniform(0.3, 0.9, n) * (r + rad[0]))[:, None] * d
    a.set_body(mass=m, radius=r, position=x, velocity=np.zeros((n, 3)))
    J = a.jacobian(link=10).double()
    a.world_step()
    w = a.body_state().double()
    F = w[:, 6:7] * w[:, 3:6] / H                                       # m dv / h, dv = v (it started at rest)
    tau = -torch.einsum("nij,ni->nj", J[:, 0:3], F)
    b.world_step(joint_torques=tau.float())
    c.world_step()
    da, db, dc = (dyn_words(e).astype(np.float64) for e in (a, b, c))
    dq, dqd = np.abs(da[0:6] - db[0:6]).max(), np.abs(da[6:12] - db[6:12]).max()
    effect = np.abs(db[6:12] - dc[6:12]).max(axis=0)
    print(f"sphere vs J^T (-F) on the GPU: |dq| {dq:.3e} of {Q_TOL:.1e}, |dqd| {dqd:.3e} of {QD_TOL:.1e}; F moves qd by {effect.max():.3e} at most, "
          f"{np.median(effect):.3e} in the median env; |F| {float(F.norm(dim=1).min()):.1f} .. {float(F.norm(dim=1).max()):.1f}")
    assert effect.max() > 10 * QD_TOL and np.median(effect) > 10 * QD_TOL
    assert dq <= Q_TOL and dqd <= QD_TOL
    for env in (a, b, c):
        env.close()


# ---- 3. rest ------------------------------------------------------------------------------------------------------------------------
def test_a_sphere_comes_to_rest_on_the_ground():
    """after 200 world steps z = ground_z + radius - m g / kp to 1e-5 (about 80 float32 ulps at z = 0.5) and |v| <= 1e-4: mass 1
    on the default spring is damped at ratio 0.56 and settles within tens of sub-steps"""
    n = 97
    env = make("C", n)
    m, r, kp, g = 1.0, 0.5, 2000.0, 9.81
    env.set_body(mass=m, radius=r, position=(60.0, 30.0, r), velocity=(0.0, 0.0, 0.0))      # beyond the arm and the box
    for _ in range(200):
        env.world_step()
    w = body_words(env).astype(np.float64)
    dz, speed = np.abs(w[2] - (0.0 + r - m * g / kp)).max(), np.linalg.norm(w[3:6], axis=0).max()
    print(f"rest: |z - (ground_z + radius - m g / kp)| {dz:.3e} of 1e-5, |v| {speed:.3e} of 1e-4")
    assert dz <= 1e-5 and speed <= 1e-4
    assert np.array_equal(w[0:2], np.broadcast_to(np.array([[60.0], [30.0]]), (2, n)))
    env.close()


# ---- 4. envs with mass 0 ------------------------------------------------------------------------------------------------------------
def test_envs_without_a_sphere_step_like_a_handle_without_one():
    """Their eight words come back bit for bit, and their joints agree with a sphere-less handle's plain step within Q_TOL / QD_TOL
    (tests/bars.py: tighter than ROLL_OBS_TOL, the bar of two instantiations of one text under fp contraction, which these are)."""
    n, family = 1000, "A"
    a, b = make(family, n), make(family, n, sphere=False)
    q, qd = cases.states(family, command_r(a))
    w0 = cases.spheres(family, q)
    w0[6, ::2] = 0.0                                                    # every other env has none ..
    w0[6, 1] = -1.0                                                     # .. and a negative mass is none too
    for env in (a, b):
        load_joints(env, q, qd)
    a.set_body_state(dev(w0.T))
    for step in range(cases.STEPS):
        b.set_dyn_state(a.get_dyn_state())
        a.world_step()
        b.world_step()
        da, db = dyn_words(a).astype(np.float64), dyn_words(b).astype(np.float64)
        gone = w0[6] <= 0
        dq, dqd = np.abs(da[0:6, gone] - db[0:6, gone]).max(), np.abs(da[6:12, gone] - db[6:12, gone]).max()
        moved = np.abs(da[6:12, ~gone] - db[6:12, ~gone]).max()
        print(f"mass 0, step {step}: |dq| {dq:.3e} of {Q_TOL:.1e}, |dqd| {dqd:.3e} of {QD_TOL:.1e}; the envs with a sphere differ by {moved:.3e}")
        assert dq <= Q_TOL and dqd <= QD_TOL
        assert np.array_equal(body_words(a)[:, gone].view(np.uint32), w0[:, gone].view(np.uint32))
    assert moved > 10 * QD_TOL
    a.close(); b.close()


# ---- 5. the state calls -------------------------------------------------------------------------------------------------------------
def test_body_state_round_trip_and_mask():
    n = 97
    env = make("A", n)
    assert not env.body_state().any()                                  # zero-filled: every env inert
    rng = np.random.default_rng(5)
    w = dev(rng.normal(size=(n, 8)))
    env.set_body_state(w)
    assert torch.equal(bits(env.body_state()), bits(w))
    w2 = dev(rng.normal(size=(n, 8)))
    mask = torch.zeros(n, dtype=torch.bool, device="cuda:0")
    mask[[0, 5, 63, 64, 96]] = True
    env.set_body_state(w2, mask=mask)
    got = env.body_state()
    assert torch.equal(bits(got[mask]), bits(w2[mask])) and torch.equal(bits(got[~mask]), bits(w[~mask]))
    sd = env.state_dict()
    assert np.array_equal(sd["body"], got.cpu().numpy())
    env.set_body_state(w)
    env.load_state_dict(sd)
    assert torch.equal(bits(env.body_state()), bits(got))
    env.set_body(False)
    assert "body" not in env.state_dict()
    assert torch.equal(bits(env.body_state()), bits(got))             # disabled, the buffer is kept
    env.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
def _refused(code, text, fn, *args):
    with pytest.raises(_lib().PnrError) as ei:
        fn(*args)
    assert ei.value.code == code and text in str(ei.value), (ei.value.code, str(ei.value))


def test_refusals():
    L = _lib()
    n = 64
    kin = kin_env(n, 3)
    _refused(UNSUPPORTED, "dynamics mode only", kin.set_body)
    _refused(INVALID, "before pnr_set_body_params", kin.body_state)
    kin.close()
    env = make("A", n, sphere=False)
    _refused(INVALID, "before pnr_set_body_params", env.body_state)
    _refused(INVALID, "before pnr_set_body_params", env.set_body_state, torch.zeros((n, 8), device="cuda:0"))
    for bad in (dict(contact_kp=0.0), dict(contact_kd=-1.0), dict(friction=-0.1), dict(linear_damping=-1.0), dict(slip_eps=0.0)):
        _refused(INVALID, "pnr_set_body_params", env.set_body, bad)
    _refused(INVALID, "before pnr_set_body_params", env.body_state)    # a refused call enabled nothing
    env.set_body()
    buf = torch.zeros(8 * n + 4, device="cuda:0")
    off = C.c_void_p(buf.data_ptr() + 4)
    stream = env._stream()
    for fn, args, name in ((env.lib.pnr_set_body_state, (off, None, stream), "words"), (env.lib.pnr_get_body_state, (off, stream), "out")):
        assert fn(env._h, *args) == INVALID
        assert f"{name} must be 16-byte aligned" in env.lib.pnr_last_error(env._h).decode()
    # the combinations that are not built name the sphere
    spec, wr, tq = [(10, "world")], torch.zeros((n, 1, 9), device="cuda:0"), torch.zeros((n, 6), device="cuda:0")
    _refused(UNSUPPORTED, "moving sphere", lambda: env.world_step(link_wrenches=(spec, wr)))
    _refused(UNSUPPORTED, "moving sphere", env.joint_states)
    env.set_joint_motor(2, L.CONTROL_VELOCITY_CONSTRAINT, target_velocity=0.1, max_force=50.0)
    _refused(UNSUPPORTED, "moving sphere", env.world_step)
    _refused(UNSUPPORTED, "moving sphere", lambda: env.world_step(motor_targets=torch.zeros((n, 12), device="cuda:0")))
    _refused(UNSUPPORTED, "constraint motor", lambda: env.world_step(joint_torques=tq))
    d0 = env.get_dyn_state().clone()
    env.set_body(False)                                                 # disabled: the refused calls work again
    env.world_step()
    env.world_step(motor_targets=torch.zeros((n, 12), device="cuda:0"))
    env.joint_states()
    env.set_joint_motor(2, L.CONTROL_VELOCITY, target_velocity=0.0)
    env.world_step(link_wrenches=(spec, wr))
    assert not torch.equal(env.get_dyn_state()[0:12], d0[0:12])
    env.close()


# ---- 7. the facade ------------------------------------------------------------------------------------------------------------------
def test_facade_sphere_falls_lands_and_is_read_and_written():
    from pioneer_amd import EngineConfig, PioneerKinematicEnv, SimulationConfig
    quat = (0.0, 0.0, 0.0, 1.0)
    env = PioneerKinematicEnv(simulation_config=SimulationConfig(gravity=9.81), engine_config=EngineConfig(mode="dynamic", renderer="engine"))
    env.reset()
    sc = env.scene
    sc.create_body_plane("floor", 0.0, (0.0, 0.0, 1.0), (0.0, 0.0, 0.0), quat)
    sc.create_body_sphere("ball", True, 2.0, 0.5, (40.0, 20.0, 1.5), quat)
    ball = sc.items_by_name["ball"]
    assert ball.pose().position == (40.0, 20.0, 1.5) and ball.velocity().linear == (0.0, 0.0, 0.0)
    env.world.step()
    z1, vz1 = ball.pose().position[2], ball.velocity().linear[2]
    t = env.world.step_time
    print(f"facade: after one step z {z1:.6f} vz {vz1:.6f}; free fall gives {1.5 - 0.5 * 9.81 * t * (t + 1 / 240):.6f} {-9.81 * t:.6f}")
    assert abs(vz1 + 9.81 * t) <= 1e-5 and abs(z1 - (1.5 - 0.5 * 9.81 * t * (t + 1.0 / 240))) <= 1e-5     # semi-implicit Euler, 10 sub-steps
    for _ in range(150):
        env.world.step()
    z, v = ball.pose().position[2], ball.velocity().linear
    print(f"facade: landed at z {z:.6f} (rest {0.5 - 2.0 * 9.81 / 2000.0:.6f}), v {v}")
    assert abs(z - (0.5 - 2.0 * 9.81 / 2000.0)) <= 1e-4 and max(abs(c) for c in v) <= 1e-3
    rgb = env.render("rgb_array")
    assert rgb.ndim == 3
    ball.reset_pose((41.0, 19.0, 3.0), quat)
    assert ball.pose().position == (41.0, 19.0, 3.0) and ball.velocity().linear == (0.0, 0.0, 0.0)
    sc.create_body_box("crate", True, 0.0, (1.0, 1.0, 1.0), (30.0, -20.0, 1.0), quat)      # the engine is rebuilt: the sphere carries over
    assert ball.pose().position == (41.0, 19.0, 3.0)
    with pytest.raises(AssertionError):
        sc.create_body_sphere("second", True, 1.0, 0.5, (0.0, 0.0, 5.0), quat)
    with pytest.raises(AssertionError):
        sc.create_body_box("heavy", True, 1.0, (1.0, 1.0, 1.0), (0.0, 0.0, 5.0), quat)
    with pytest.raises(AssertionError):
        sc.create_body_sphere("ghost", False, 1.0, 0.5, (0.0, 0.0, 5.0), quat)
    env.close()
    kin = PioneerKinematicEnv()
    kin.reset()
    with pytest.raises(AssertionError):
        kin.scene.create_body_sphere("ball", True, 2.0, 0.5, (40.0, 20.0, 1.5), quat)
    kin.close()
