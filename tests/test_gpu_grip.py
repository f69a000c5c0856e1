"""GPU tests of the grip (pnr_set_body_grip_params / pnr_set_body_grip / pnr_get_body_grip and the world step's kWorldGrip forms;
PioneerVectorEnv.set_body_grip / body_grip / grip_anchor, the facade's create_constraint) against the float64 reference of
tests/grip_ref.py, on the inputs of tests/grip_cases.py.

Bars.  Joints: Q_TOL / QD_TOL (tests/bars.py).  The sphere's position and velocity and the reported force: 4 x the reference's own
float32-storage deviation on the same inputs (cases.grip_bars), the position bar capped at PTR_TOL.  Hold: 1.5 m g / grip_kp after
the K world steps the reference needs (cases.hold_steps).  Carry: 1.5 x the reference's own worst distance (cases.carry_reference).
tests/test_grip_cpu.py asserts the conditions on the inputs.  Every test prints its figures before it asserts.
MEASURED ON AN MI355X (worst over both sizes, the three call forms and three world steps; DESIGN.md 3w has the table):
    G1  joints |dq| 9.2e-7 |dqd| 3.1e-5; sphere |dx| 8.3e-6 of 3.0e-5, |dv| 6.7e-4 of 9.4e-4; force |dF| 1.7e-2 of 3.3e-2 (|F| up to 5115)
    G2  joints |dq| 8.0e-7 |dqd| 3.7e-5; sphere |dx| 9.1e-6 of 3.4e-5, |dv| 2.3e-4 of 4.2e-4; force |dF| 1.5e-2 of 2.5e-2 (|F| up to 300)
    saturation |F| 1 +- 1e-7; hold after K = 20 steps 1.1785e-2 (reference 1.1786e-2) of 1.4715e-2; carry 7.4227e-2 (reference 7.4225e-2, bar 1.5 x)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import grip_cases as cases
import grip_ref as gref
import link_kinematics_ref as lk
import moving_sphere_cases as msc
import moving_sphere_ref as sref
from bars import Q_TOL, QD_TOL
from gpu_support import bits, dev, dyn_words, engine_config_from_oracle_names, kin_env, lib as _lib, load_joints

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5


def make(family, n, grip=True):
    """the family's env, reset, with the sphere enabled and, with `grip`, the grip under the family's params (every env released)"""
    from pioneer_amd import PioneerVectorEnv, SimulationConfig
    f = cases.base_family(family)
    env = PioneerVectorEnv(n, device="cuda:0", seed=f["seed"], simulation_config=SimulationConfig(gravity=f["gravity"], frame_skip=cases.FRAME_SKIP),
                           engine_config=engine_config_from_oracle_names(dict(f["dyn"]), auto_reset=False, max_episode_steps=0))
    env.reset()
    env.set_body()
    if grip:
        env.set_body_grip(cases.FAMILIES[family]["grip"])
    return env


def held_env(case, max_force=None):
    """HOLD's or CARRY's env: the arm at its command state at rest, the sphere gripped at its anchor point at rest"""
    from pioneer_amd import PioneerVectorEnv, SimulationConfig
    env = PioneerVectorEnv(case["n"], device="cuda:0", seed=case["seed"], simulation_config=SimulationConfig(gravity=case["gravity"], frame_skip=cases.FRAME_SKIP),
                           engine_config=engine_config_from_oracle_names(dict(case["dyn"]), auto_reset=False, max_episode_steps=0))
    env.reset()
    load_joints(env, command_r(env), None)
    env.set_body(mass=case["mass"], radius=case["radius"], position=(0.0, 0.0, 0.0), velocity=(0.0, 0.0, 0.0))
    env.set_body_grip(max_force=case["max_force"] if max_force is None else max_force)
    env.set_body(position=env.grip_anchor())
    return env


def command_r(env):
    return env.get_state().view(torch.float32)[12:18].T.cpu().numpy()


def body_words(env):
    return env.body_state().T.cpu().numpy()


def grip_words(env):
    """[4, N] float32 on the host"""
    return env.body_grip().T.cpu().numpy()


def call(env, form, tq, tg):
    if form == "plain":
        env.world_step()
    elif form == "torques":
        env.world_step(joint_torques=tq)
    else:
        env.world_step(joint_torques=tq, motor_targets=tg, motor_joints=cases.TARGET_JOINTS)


def load_case(env, family):
    """the family's inputs into the env: (q, qd, sphere words, max_force, tau, targets) on the host"""
    base = cases.FAMILIES[family]["base"]
    r = command_r(env)
    q, qd = msc.states(base, r)
    load_joints(env, q, qd)
    w0, fmax = cases.spheres(family, q, qd)
    env.set_body_state(dev(w0.T))
    env.set_body_grip(max_force=fmax)
    return w0, fmax, msc.joint_torques(base, env.num_envs), msc.targets(base, r)


def anchor_distance(env):
    return (env.body_state()[:, 0:3] - env.grip_anchor()).norm(dim=1)


# ---- 1. against the reference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", cases.FORMS)
@pytest.mark.parametrize("family", list(cases.FAMILIES))
@pytest.mark.parametrize("n", cases.SIZES)
def test_world_step_with_a_grip_against_the_reference(n, family, form):
    """STEPS world steps, the reference re-synchronised with the engine before each.  At n = 1000 the reference follows every 8th
    env and the partial last wave."""
    env = make(family, n)
    idx = cases.followed(n)
    orc = cases.make_oracle(family, len(idx), reset=False)
    orc.load_state_words(env.get_state().cpu().numpy().view(np.uint32)[:, idx])
    w0, fmax, tau, tg = load_case(env, family)
    tq, tgd = dev(tau), dev(tg)
    te, tt, joints = cases.form_inputs(form, tau[idx], tg[idx])
    bar_x, bar_v, bar_f = cases.grip_bars(family)
    g0 = grip_words(env)
    assert np.array_equal(g0[0], fmax) and not g0[1:4].any()
    worst = dict(q=0.0, qd=0.0, x=0.0, v=0.0, f=0.0)
    for step in range(cases.STEPS):
        orc.load_dyn_words(dyn_words(env)[:, idx])
        before, gb = body_words(env), grip_words(env)
        s = sref.from_words(before[:, idx])
        res = gref.world_step(orc, cases.TRACK, sphere=s, max_force=fmax[idx].astype(np.float64), grip_params=cases.FAMILIES[family]["grip"],
                              tau_ext=te, targets=tt, joints=joints)
        live, on = s["m"] > 0, gref.held(s, fmax[idx])
        first = res["records"][0]
        if step == 0:
            capped = (first["held"] & (np.linalg.norm(first["grip_raw"], axis=1) > fmax[idx])).mean()
            print(f"family {family} n={n} {form}: {on.mean():.2%} of the followed envs are held ({capped:.2%} at their cap), "
                  f"{first['on_arm'].mean():.2%} touch the arm, {1 - live.mean():.2%} have no sphere")
        call(env, form, tq, tgd)
        e = dyn_words(env)[:, idx].astype(np.float64)
        after, ga = body_words(env), grip_words(env)
        got = sref.from_words(after[:, idx])
        dq, dqd = np.abs(e[0:6].T - orc.dstate["q"]).max(), np.abs(e[6:12].T - orc.dstate["qd"]).max()
        dx, dv = np.abs(got["x"] - s["x"])[live].max(), np.abs(got["v"] - s["v"])[live].max()
        df = np.abs(ga[1:4, idx].T.astype(np.float64) - res["force"])[on].max()
        for k, v in dict(q=dq, qd=dqd, x=dx, v=dv, f=df).items():
            worst[k] = max(worst[k], float(v))
        print(f"family {family} n={n} {form} step={step}: |dq| {dq:.3e} of {Q_TOL:.1e}, |dqd| {dqd:.3e} of {QD_TOL:.1e}, sphere |dx| {dx:.3e} of "
              f"{bar_x:.3e}, |dv| {dv:.3e} of {bar_v:.3e}, force |dF| {df:.3e} of {bar_f:.3e} (|F| up to {np.abs(res['force']).max():.1f})")
        gone, released = before[6] <= 0, ~(fmax > 0)                   # every env of the batch, followed or not
        assert np.array_equal(after[:, gone].view(np.uint32), before[:, gone].view(np.uint32)), "an env without a sphere had its words written"
        assert np.array_equal(ga[:, gone].view(np.uint32), gb[:, gone].view(np.uint32)), "an env without a sphere had its grip words written"
        assert not ga[1:4, released].any(), "a released env reports a force"
        assert np.array_equal(ga[0].view(np.uint32), fmax.view(np.uint32)), "max_force is never written by the step"
        assert np.array_equal(after[6:8].view(np.uint32), before[6:8].view(np.uint32)), "mass and radius are never written"
        assert dq <= Q_TOL and dqd <= QD_TOL, (family, n, form, step, dq, dqd)
        assert dx <= bar_x and dv <= bar_v, (family, n, form, step, dx, bar_x, dv, bar_v)
        assert df <= bar_f, (family, n, form, step, df, bar_f)
    print(f"family {family} n={n} {form} WORST: |dq| {worst['q']:.3e} |dqd| {worst['qd']:.3e} sphere |dx| {worst['x']:.3e} |dv| {worst['v']:.3e} "
          f"force |dF| {worst['f']:.3e}")
    env.close()


# ---- 2. batch independence -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "targets"])
@pytest.mark.parametrize("family", list(cases.FAMILIES))
def test_an_env_does_not_depend_on_the_batch_around_it(family, form):
    """the results of n = 97 are the first 97 rows of n = 1000, bit for bit"""
    out = []
    for n in cases.SIZES:
        env = make(family, n)
        _, _, tau, tg = load_case(env, family)
        for _ in range(cases.STEPS):
            call(env, form, dev(tau), dev(tg))
        out.append((dyn_words(env)[0:12], body_words(env), grip_words(env)))
        env.close()
    small, big = out
    for a, b, what in zip(small, big, ("joints", "sphere", "grip")):
        assert np.array_equal(a.view(np.uint32), b[:, :cases.SIZES[0]].view(np.uint32)), what
    assert np.abs(small[2][1:4]).max() > 1.0


# ---- 3. the grip disabled is the handle that never had one -----------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(cases.FAMILIES))
def test_grip_disabled_steps_as_a_handle_that_never_gripped(family):
    n = cases.SIZES[0]
    a, b = make(family, n, grip=False), make(family, n)
    w0, fmax, tau, tg = load_case(b, family)
    load_joints(a, *msc.states(cases.FAMILIES[family]["base"], command_r(a)))
    a.set_body_state(dev(w0.T))
    d0, s0 = b.get_dyn_state().clone(), b.body_state().clone()
    assert torch.equal(bits(a.get_dyn_state()), bits(d0)) and torch.equal(bits(a.body_state()), bits(s0))
    b.world_step()                                                      # gripped, stepped ..
    assert not torch.equal(bits(b.body_state()), bits(s0)) and np.abs(grip_words(b)[1:4]).max() > 1.0
    sd = b.state_dict()                                                 # (the grip's words are part of the state dict while it is enabled)
    assert np.array_equal(sd["grip"], b.body_grip().cpu().numpy()) and np.array_equal(sd["grip"][:, 0], fmax)
    b.set_body_grip(max_force=0.0)
    b.load_state_dict(sd)
    assert np.array_equal(grip_words(b)[0], fmax) and not grip_words(b)[1:4].any()
    b.set_dyn_state(d0)                                                 # .. restored ..
    b.set_body_state(s0)
    b.set_body_grip(False)                                              # .. and disabled; max_force stays in the buffer, unread
    assert np.array_equal(grip_words(b)[0], fmax)
    for step, form in enumerate(cases.FORMS):
        call(a, form, dev(tau), dev(tg))
        call(b, form, dev(tau), dev(tg))
        assert torch.equal(bits(a.get_dyn_state()[0:12]), bits(b.get_dyn_state()[0:12])), (step, form)
        assert torch.equal(bits(a.body_state()), bits(b.body_state())), (step, form)
    a.close(); b.close()


# ---- 4. saturation -------------------------------------------------------------------------------------------------------------------
def test_a_grip_weaker_than_the_weight_reports_its_cap_and_lets_the_sphere_sink():
    """mass 2 under gravity, max_force 1 < m g, the sphere 0.5 below its anchor: F_r is about 1000, so F is capped from the first
    sub-step on; the reported |F| is 1 to 1e-5 relative and the sphere is lower after one world step"""
    env = held_env(cases.HOLD, max_force=1.0)
    w = env.body_state().clone()
    w[:, 2] -= 0.5
    env.set_body_state(w)
    z0 = env.body_state()[:, 2].clone()
    env.world_step()
    g = env.body_grip().double()
    size = g[:, 1:4].norm(dim=1)
    sunk = z0 - env.body_state()[:, 2]
    print(f"saturation: |F| in {float(size.min()):.7f} .. {float(size.max()):.7f} of 1; the sphere sinks by {float(sunk.min()):.4f} .. {float(sunk.max()):.4f}")
    assert float((size - 1.0).abs().max()) <= 1e-5
    assert bool((sunk > 0).all())
    assert bool((g[:, 3] > 0.9).all())                                  # it pulls upwards, towards the anchor
    env.close()


# ---- 5. hold at rest -----------------------------------------------------------------------------------------------------------------
def test_a_gripped_sphere_hangs_at_its_anchor():
    """the CPU test's bound, 1.5 m g / grip_kp, after the K world steps the reference needs (tests/test_grip_cpu.py)"""
    K, ref_err = cases.hold_steps()
    env = held_env(cases.HOLD)
    orc, s, _ = cases.held_oracle(cases.HOLD)
    da = float(np.abs(env.body_state()[:, 0:3].double().cpu().numpy() - s["x"]).max())      # grip_anchor() against the reference's p_a
    print(f"hold: grip_anchor() differs from the reference's anchor point by {da:.3e}")
    assert da <= 1e-4
    for _ in range(K):
        env.world_step()
    err = anchor_distance(env)
    g = env.body_grip().double()
    print(f"hold: after K = {K} world steps |x - p_a| {float(err.max()):.4e} (the reference: {ref_err:.4e}) of {cases.hold_bound():.4e}; "
          f"F_z {float(g[:, 3].min()):.3f} .. {float(g[:, 3].max()):.3f}, m g = {cases.HOLD['mass'] * cases.G:.3f}")
    assert float(err.max()) <= cases.hold_bound()
    assert float((g[:, 3] - cases.HOLD["mass"] * cases.G).abs().max()) <= 0.5 * cases.HOLD["mass"] * cases.G      # the grip carries the weight
    env.close()


# ---- 6. carry ------------------------------------------------------------------------------------------------------------------------
def test_a_gripped_sphere_follows_the_arm():
    """per-env motor targets stepped towards a pose 0.3 rad away over 20 world steps: the worst |x - grip_anchor()| over the
    trajectory is at most 1.5 x the same quantity on the reference's run of the same inputs"""
    ref_worst = cases.carry_reference()
    env = held_env(cases.CARRY)
    r = command_r(env)
    q0 = dyn_words(env)[0:6].copy()
    worst = 0.0
    for step in range(cases.CARRY["steps"]):
        env.world_step(motor_targets=dev(cases.carry_targets(r, step)))
        worst = max(worst, float(anchor_distance(env).max()))
    turned = np.abs(dyn_words(env)[0:6] - q0).max(axis=0)
    print(f"carry: worst |x - p_a| {worst:.4e}, on the reference {ref_worst:.4e} (x 1.5 = {1.5 * ref_worst:.4e}); the joints turned by up to "
          f"{turned.min():.3f} .. {turned.max():.3f} rad")
    assert turned.min() > 0.1                                           # the arm did move
    assert worst <= 1.5 * ref_worst
    env.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def _refused(code, text, fn, *args, **kw):
    with pytest.raises(_lib().PnrError) as ei:
        fn(*args, **kw)
    assert ei.value.code == code and text in str(ei.value), (ei.value.code, str(ei.value))


def test_refusals_change_nothing():
    L = _lib()
    n = 64
    kin = kin_env(n, 3)
    _refused(UNSUPPORTED, "dynamics mode only", kin.set_body_grip)
    _refused(INVALID, "before pnr_set_body_grip_params", kin.body_grip)
    kin.close()
    assert L.load_library().pnr_set_body_grip_params(None, None) == INVALID and L.load_library().pnr_get_body_grip(None, None, None) == INVALID
    assert L.load_library().pnr_body_grip_params_default(None) == INVALID
    family = "G1"
    env, twin = make(family, n, grip=False), make(family, n)
    from pioneer_amd import PioneerVectorEnv, SimulationConfig
    f = cases.base_family(family)
    fresh = PioneerVectorEnv(n, device="cuda:0", seed=f["seed"], simulation_config=SimulationConfig(gravity=f["gravity"], frame_skip=cases.FRAME_SKIP),
                             engine_config=engine_config_from_oracle_names(dict(f["dyn"]), auto_reset=False, max_episode_steps=0))
    fresh.reset()
    _refused(INVALID, "before pnr_set_body_params", fresh.set_body_grip)       # no sphere buffer yet
    _refused(INVALID, "before pnr_set_body_grip_params", fresh.body_grip)
    fresh.close()
    _refused(INVALID, "before pnr_set_body_grip_params", env.body_grip)
    _refused(INVALID, "before pnr_set_body_grip_params", lambda: env._chk(env.lib.pnr_set_body_grip(env._h, C.c_void_p(16), None, env._stream())))
    for bad in (dict(grip_kp=0.0), dict(grip_kp=-5.0), dict(grip_kd=-1.0), dict(grip_kp=float("inf")), dict(anchor=(0.0, float("nan"), 0.0)),
                dict(direction=(float("inf"), 0.0, 0.0)), dict(direction=(1e-30, 0.0, 0.0))):
        _refused(INVALID, "pnr_set_body_grip_params", env.set_body_grip, bad)
    p = L.PnrBodyGripParams()
    assert env.lib.pnr_body_grip_params_default(p) == 0 and p.struct_size == C.sizeof(L.PnrBodyGripParams)
    assert abs(sum(c * c for c in p.direction) - 1.0) <= 1e-6 and p.direction[1] == 0.0 and tuple(p.anchor) == (0.0, 0.0, 0.0)
    assert p.grip_kp != p.grip_kp and p.grip_kd != p.grip_kd            # NaN: the sphere's contact gains
    p.struct_size = 12
    assert env.lib.pnr_set_body_grip_params(env._h, p) == INVALID and "struct_size" in env.lib.pnr_last_error(env._h).decode()
    _refused(INVALID, "before pnr_set_body_grip_params", env.body_grip)        # a refused call enabled and allocated nothing
    # from here on: the same grip as the twin's, then refused calls, then one step on both
    env.set_body_grip(cases.FAMILIES[family]["grip"])
    for e in (env, twin):
        load_case(e, family)
    g0 = env.body_grip().clone()
    _refused(INVALID, "pnr_set_body_grip_params", env.set_body_grip, dict(grip_kp=-1.0))
    buf = torch.zeros(4 * n + 4, device="cuda:0")
    stream = env._stream()
    assert env.lib.pnr_get_body_grip(env._h, C.c_void_p(buf.data_ptr() + 4), stream) == INVALID
    assert "out must be 16-byte aligned" in env.lib.pnr_last_error(env._h).decode()
    assert env.lib.pnr_get_body_grip(env._h, None, stream) == INVALID and "null out" in env.lib.pnr_last_error(env._h).decode()
    assert env.lib.pnr_set_body_grip(env._h, None, None, stream) == INVALID and "null max_force" in env.lib.pnr_last_error(env._h).decode()
    assert env.lib.pnr_set_body_grip(env._h, C.c_void_p(buf.data_ptr() + 2), None, stream) == INVALID
    assert "max_force must be 4-byte aligned" in env.lib.pnr_last_error(env._h).decode()
    # what the sphere refuses stays refused, in the sphere's messages
    spec, wr, tq = [(10, "world")], torch.zeros((n, 1, 9), device="cuda:0"), torch.zeros((n, 6), device="cuda:0")
    _refused(UNSUPPORTED, "moving sphere", lambda: env.world_step(link_wrenches=(spec, wr)))
    _refused(UNSUPPORTED, "moving sphere", env.joint_states)
    env.set_joint_motor(2, L.CONTROL_VELOCITY_CONSTRAINT, target_velocity=0.1, max_force=50.0)
    _refused(UNSUPPORTED, "moving sphere", env.world_step)
    _refused(UNSUPPORTED, "moving sphere", lambda: env.world_step(motor_targets=torch.zeros((n, 12), device="cuda:0")))
    _refused(UNSUPPORTED, "constraint motor", lambda: env.world_step(joint_torques=tq))
    assert torch.equal(bits(env.body_grip()), bits(g0)) and torch.equal(bits(env.body_state()), bits(twin.body_state()))
    assert torch.equal(bits(env.get_dyn_state()), bits(twin.get_dyn_state()))
    twin.set_joint_motor(2, L.CONTROL_VELOCITY, target_velocity=0.1)
    env.set_joint_motor(2, L.CONTROL_VELOCITY, target_velocity=0.1)
    env.world_step()
    twin.world_step()
    assert torch.equal(bits(env.get_dyn_state()), bits(twin.get_dyn_state())) and torch.equal(bits(env.body_state()), bits(twin.body_state()))
    assert torch.equal(bits(env.body_grip()), bits(twin.body_grip())) and float(env.body_grip()[:, 1:4].abs().max()) > 1.0
    env.close(); twin.close()


# ---- 8. the facade -------------------------------------------------------------------------------------------------------------------
def test_facade_pick_hold_and_drop():
    from pioneer_amd import PioneerKinematicEnv, SimulationConfig
    K, _ = cases.hold_steps()
    quat = (0.0, 0.0, 0.0, 1.0)
    mass, radius = cases.HOLD["mass"], cases.HOLD["radius"]
    env = PioneerKinematicEnv(simulation_config=SimulationConfig(gravity=cases.HOLD["gravity"]),
                              engine_config=engine_config_from_oracle_names(dict(cases.HOLD["dyn"])))
    env.reset()
    sc = env.scene
    pointer = sc.links_by_name["robot:pointer"]
    # hang the ball below the pointer: the world's -z in the pointer's frame
    down = tuple(lk.matrix_from_quat(np.array([pointer.pose().orientation]))[0].T @ np.array([0.0, 0.0, -1.0]))
    start = np.array(pointer.pose().position) + np.array([0.0, 0.0, -(radius + cases.POINTER_RADIUS)])
    sc.create_body_sphere("ball", True, mass, radius, tuple(start), quat)
    ball = sc.items_by_name["ball"]
    with pytest.raises(AssertionError):
        sc.create_constraint(sc.links_by_name["robot:arm1"], ball, 100.0)
    with pytest.raises(AssertionError):
        sc.create_constraint(pointer, pointer, 100.0)
    cid = sc.create_constraint(pointer, ball, 1e4, direction=down)
    with pytest.raises(AssertionError):
        sc.create_constraint(pointer, ball, 1e4)
    for _ in range(K):
        env.world.step()
    anchor = env._vec.grip_anchor()[0].double().cpu().numpy()
    err = float(np.linalg.norm(np.array(ball.pose().position) - anchor))
    force = sc.constraint_state(cid)
    print(f"facade: after K = {K} steps |x - p_a| {err:.4e} of {cases.hold_bound():.4e}; constraint_state {force}, m g = {mass * cases.G:.3f}")
    assert err <= cases.hold_bound()
    assert any(c != 0.0 for c in force) and abs(force[2] - mass * cases.G) <= 0.5 * mass * cases.G
    sc.change_constraint(cid, 5e3)
    assert float(env._vec.body_grip()[0, 0]) == 5e3 and sc.constraint_state(cid) == (0.0, 0.0, 0.0)      # the setter zeroes the report
    z0 = ball.pose().position[2]
    sc.remove_constraint(cid)
    env.world.step()
    z1 = ball.pose().position[2]
    print(f"facade: released, one step lowers the ball from z {z0:.5f} to {z1:.5f}")
    assert z1 < z0 and float(env._vec.body_grip()[0, 0]) == 0.0
    with pytest.raises(AssertionError):
        sc.constraint_state(cid)
    cid2 = sc.create_constraint(pointer, ball, 1e4, direction=down)      # .. and it can be picked up again
    assert cid2 == cid
    env.close()
