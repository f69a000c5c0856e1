"""GPU tests of pnr_get_joint_states (PioneerVectorEnv.joint_states, the facade's Joint.state / Scene.joint_states) against the
float64 reference of tests/joint_state_ref.py, on the inputs and to the bars of tests/joint_state_cases.py (FLOOR_MARGIN = 8 times
the measured float32 floors, per quantity, joint, call form and contact state, the motor torque's capped at 1e-3 of its median; the constraint cases to the project's velocity bar
of a sub-step).  tests/test_joint_state_cpu.py asserts what those bars rest on.  Every test prints its figures before it asserts.
MEASURED VALUES ON AN MI355X: see DESIGN.md 3n (the worst error of any quantity was 0.32 of its bar).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import constraint_motor_cases as ccases
import external_force_cases as xcases
import joint_state_cases as cases
import joint_state_ref as ref
import oracle_cases as ocases
from bars import QD_TOL
from gpu_support import bits, dev, dyn_env, dyn_words, lib as _lib, load_joints, set_motors, words

pytestmark = pytest.mark.gpu

H = cases.H
SENTINEL = -7.25
FORMS = {"ext": (True, True), "wrench": (True, False), "torque": (False, True), "plain": (False, False)}


def scenario(name, n, frame_skip=None):
    """(env, inputs for the whole batch as device tensors and arrays) of a family, `hold` or a constraint case, its states loaded"""
    if name in cases.CONSTRAINT:
        c = ccases.CASES[name]
        env = dyn_env(n, c["seed"], ccases.GRAVITY, c["frame_skip"], **c["engine"])
        for act in ocases.command_actions(c["seed"], c.get("command_steps", 0), n, env.a_max):
            env.vector_step(torch.from_numpy(act).cuda())
        set_motors(env, c["motors"])
        q, qd = ccases.states(name, n, 0)
        I = dict(motors=c["motors"], specs=(), wrenches=None, tau=None)
    elif name == "hold":
        from inverse_dynamics_cases import HOLD_SEED
        env = dyn_env(n, HOLD_SEED, 9.81, frame_skip or 10, randomize=True, rand_friction=(0.0, 0.0), rand_damping=(0.0, 0.0))
        orc = cases.hold_oracle(n)
        assert np.array_equal(dyn_words(env)[12:35], orc.dyn_words()[12:35]), "the engine's link draws are the oracle's"
        _, I = cases.hold_inputs(n, orc)
        set_motors(env, I["motors"])
        q, qd = I["q"], I["qd"]
    else:
        f = xcases.FAMILIES[name]
        env = dyn_env(n, f["seed"], f["gravity"], frame_skip or xcases.FRAME_SKIP, **f["engine"])
        set_motors(env, f["motors"])
        r_cmd = env.get_state().view(torch.float32)[12:18].T.cpu().numpy()
        q, qd = xcases.states(name, r_cmd)
        I = dict(motors=f["motors"], specs=f["specs"], wrenches=xcases.wrenches(name, q), tau=xcases.joint_torques(name, n))
    load_joints(env, q, qd)
    I.update(q=q, qd=qd)
    return env, I


_REF = {}


def reference(name, n, form, env, I):
    """The float64 reference on the followed envs, computed once per (scenario, batch, form) and left unchanged."""
    key = (name, n, form)
    if key not in _REF:
        idx = cases.followed(n)
        if name in cases.CONSTRAINT:
            orc = ccases.make_oracle(name, n)
            assert np.array_equal(words(env)[:21], orc.state_words()[:21])
            assert n <= 64
        elif name == "hold":
            orc = cases.hold_oracle(len(idx))
        else:
            orc = xcases.make_oracle(name, len(idx), reset=False)
        orc.load_state_words(words(env)[:, idx])
        orc.load_dyn_words(dyn_words(env)[:, idx])
        sub = {k: (v[idx] if isinstance(v, np.ndarray) else v) for k, v in I.items()}
        R = cases.reference(orc, sub, *FORMS[form])
        R["room"] = cases.clamp_room(orc, sub, R["qdd"])
        R["scales"], R["gravity"] = orc.dstate["mass_scale"].copy(), orc.d.gravity
        _REF[key] = (idx, R)
    return _REF[key]


def query(env, I, form, **kw):
    with_w, with_t = FORMS[form]
    return env.joint_states(joint_torques=dev(I["tau"]) if with_t else None,
                            link_wrenches=(I["specs"], dev(I["wrenches"])) if with_w else None, **kw)


def against_the_reference(name, n, form):
    env, I = scenario(name, n)
    idx, R = reference(name, n, form, env, I)
    before = (env.get_state().clone(), env.get_dyn_state().clone())
    out = query(env, I, form)
    torch.cuda.synchronize()
    assert torch.equal(bits(env.get_state()), bits(before[0])) and torch.equal(bits(env.get_dyn_state()), bits(before[1])), "a query"
    joints, reaction = out["joints"].double().cpu().numpy(), out["reaction"].double().cpu().numpy()
    assert np.array_equal(joints[:, :, 0], I["q"].astype(np.float64)) and np.array_equal(joints[:, :, 1], I["qd"].astype(np.float64))
    bar = cases.bars(name, form, R["hit"])
    gf, gm = cases.split(reaction[idx])
    rf, rm = cases.split(R["reaction"])
    err = dict(qdd=np.abs(joints[idx, :, 2] - R["qdd"]), tau=np.abs(joints[idx, :, 3] - R["tau_motor"]),
               force=np.abs(gf - rf).max(axis=2), moment=np.abs(gm - rm).max(axis=2))
    ok = True
    for k in cases.QUANTITIES:
        worst = (err[k] / np.where(bar[k] > 0, bar[k], 1.0)).max()
        print(f"{name} n={n} {form} {k}: worst |error| {err[k].max():.3e}, worst error / bar {worst:.3f} "
              f"({int(R['hit'].sum())} of {len(idx)} followed envs in contact)")
        ok = ok and bool(np.all(err[k] <= bar[k]))
    assert ok, (name, n, form)
    env.close()


# ---- against the reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("n", cases.SIZES)
def test_family_c_at_every_size(n, form):
    """one lane, a short tile, a full wave, many waves with a short last tile: contacts, randomised links, four mixed records"""
    against_the_reference("C", n, form)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("family", ["A", "B", "D", "Dc"])
def test_the_other_families(family, form):
    """with C the four PHYS instantiations, each with the records and the torques, the records alone, the torques alone (external
    inputs without a record: what the facade asks after control_torque alone), and neither"""
    against_the_reference(family, 64, form)


def test_the_held_arm():
    """gravity, the holding torques and a payload on the pointer: q̈ is rounding, joint 0 carries the weight and the payload"""
    against_the_reference("hold", 64, "ext")


@pytest.mark.parametrize("case, n", [("mixed", 37), ("mixed", 64), ("subset", 64), ("scaled", 64)])
def test_constraint_motors_velocities_and_the_sweep_at_the_kernels_own_acceleration(case, n):
    """Against the reference: h |dq̈| and h |M^-1 d tau| within QD_TOL on every env.  The reaction is NOT compared with the
    reference's: q̈ is held to the coarse velocity bar only, so the reaction is checked as the function f(q, q̇, q̈_kernel), the
    float64 sweep evaluated at the kernel's own q̈, to that function's float32 bar.  A short tile too: the lanes past the batch run
    the boxed solve on a rest pose and store nothing."""
    env, I = scenario(case, n)
    idx, R = reference(case, n, "plain", env, I)
    out = query(env, I, "plain")
    joints, reaction = out["joints"].double().cpu().numpy(), out["reaction"].double().cpu().numpy()
    dv = H * np.abs(joints[:, :, 2] - R["qdd"])
    dtau = joints[:, :, 3] - R["tau_motor"]
    dvt = H * np.abs(np.einsum("nij,nj->ni", R["Minv"], dtau))
    print(f"{case} n={n}: h |dqdd| {dv.max():.3e}, h |M^-1 dtau| {dvt.max():.3e} of {QD_TOL:.1e}; |dtau| {np.abs(dtau).max():.3e} at "
          f"torques up to {np.abs(R['tau_motor']).max():.3e}")
    at = ref.newton_euler_reaction(I["q"], I["qd"], joints[:, :, 2], R["scales"], R["gravity"], R["fext"])
    F = cases.REACTION_AT_QDD[case]["plain"]["free"]
    (gf, gm), (rf, rm) = cases.split(reaction), cases.split(at)
    ef, em = np.abs(gf - rf).max(axis=2), np.abs(gm - rm).max(axis=2)
    print(f"{case} n={n}: f(q, qd, the kernel's qdd): force error / bar {(ef / (cases.FLOOR_MARGIN * F['force'])).max():.3f}, "
          f"moment error / bar {(em / (cases.FLOOR_MARGIN * F['moment'])).max():.3f}")
    assert dv.max() <= QD_TOL and dvt.max() <= QD_TOL
    assert np.all(ef <= cases.FLOOR_MARGIN * F["force"]) and np.all(em <= cases.FLOOR_MARGIN * F["moment"])
    env.close()


# ---- the step agrees with its own preview -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", cases.FAMILIES)
def test_the_step_integrates_the_acceleration_the_query_showed(family):
    """frame_skip 1: qd after world_step(same arguments) - qd before == h q̈ on every joint the clamp did not act on, within h x the
    q̈ bar plus two ulps of max(|qd|, |h q̈|); and the query left every state word as it was"""
    n = 64
    env, I = scenario(family, n, frame_skip=1)
    idx, R = reference(family, n, "ext", env, I)
    before = (env.get_state().clone(), env.get_dyn_state().clone())
    joints = query(env, I, "ext", reaction=False)["joints"].double().cpu().numpy()
    torch.cuda.synchronize()
    assert torch.equal(bits(env.get_state()), bits(before[0])) and torch.equal(bits(env.get_dyn_state()), bits(before[1]))
    env.world_step(joint_torques=dev(I["tau"]), link_wrenches=(I["specs"], dev(I["wrenches"])))
    qd0, qd1 = I["qd"].astype(np.float64), dyn_words(env)[6:12].T.astype(np.float64)
    hqdd = H * joints[:, :, 2]
    compared = R["room"] > cases.CLAMP_MARGIN
    ulp = np.spacing(np.maximum(np.abs(qd0), np.abs(hqdd)).astype(np.float32)).astype(np.float64)
    tol = H * cases.bars(family, "ext", R["hit"])["qdd"] + 2 * ulp
    err = np.abs((qd1 - qd0) - hqdd)
    print(f"family {family}: |dqd - h qdd| {err[compared].max():.3e}, worst error / tolerance {(err / tol)[compared].max():.3f}; "
          f"{int((~compared).sum())} of {compared.size} joints within the clamp's reach left out")
    assert compared.mean() > 0.98 and np.all(err[compared] <= tol[compared])
    env.close()


# ---- the outputs agree across argument forms ----------------------------------------------------------------------------------------------
def test_the_same_bits_without_the_reaction_and_from_the_callers_joints():
    n = 100
    for family in ("C", "Dc"):
        env, I = scenario(family, n)
        full = query(env, I, "ext")
        lean = query(env, I, "ext", reaction=False)
        assert set(lean) == {"joints"} and torch.equal(bits(lean["joints"]), bits(full["joints"]))
        own = torch.cat([dev(I["q"]), dev(I["qd"])], dim=1)
        given = query(env, I, "ext", joint_state=own)
        assert torch.equal(bits(given["joints"]), bits(full["joints"])) and torch.equal(bits(given["reaction"]), bits(full["reaction"]))
        other = own.clone()
        other[:, 0:6] *= 0.5
        moved = query(env, I, "ext", joint_state=other)
        assert not torch.equal(moved["joints"][:, :, 2], full["joints"][:, :, 2]), "the caller's joints are the ones read"
        env.close()


# ---- output bounds --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 37, 1000])
def test_nothing_is_written_past_the_outputs(n):
    env, I = scenario("C", n)
    guard = 256
    jbuf = torch.full((n * 24 + guard,), SENTINEL, device="cuda:0")
    rbuf = torch.full((n * 36 + guard,), SENTINEL, device="cuda:0")
    out = dict(joints=jbuf[:n * 24].view(n, 6, 4), reaction=rbuf[:n * 36].view(n, 6, 6))
    res = query(env, I, "ext", out=out)
    torch.cuda.synchronize()
    assert res["joints"].data_ptr() == jbuf.data_ptr() and res["reaction"].data_ptr() == rbuf.data_ptr()
    assert bool((jbuf[n * 24:] == SENTINEL).all()) and bool((rbuf[n * 36:] == SENTINEL).all())
    assert bool((jbuf[:n * 24] != SENTINEL).all()) and bool((rbuf[:n * 36] != SENTINEL).all()), "every output word is written"
    jbuf2 = torch.full((n * 24 + guard,), SENTINEL, device="cuda:0")
    query(env, I, "plain", reaction=False, out=dict(joints=jbuf2[:n * 24].view(n, 6, 4)))
    torch.cuda.synchronize()
    assert bool((jbuf2[n * 24:] == SENTINEL).all()) and bool((jbuf2[:n * 24] != SENTINEL).all())
    env.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_touch_no_output():
    from pioneer_amd import EngineConfig, PioneerVectorEnv
    L = _lib()
    lib = L.load_library()
    n = 8
    P = lambda t, off=0: None if t is None else C.c_void_p(t.data_ptr() + off)  # noqa: E731
    wr = torch.ones((n * 4 * 9 + 4,), device="cuda:0")
    tq = torch.ones((n * 6 + 4,), device="cuda:0")
    js = torch.zeros((n * 12 + 4,), device="cuda:0")
    jo = torch.full((n * 24 + 4,), SENTINEL, device="cuda:0")
    ro = torch.full((n * 36 + 4,), SENTINEL, device="cuda:0")

    def specs(*pairs):
        arr = (L.PnrLinkWrenchSpec * max(len(pairs), 1))()
        for j, (link, frame) in enumerate(pairs):
            arr[j].link, arr[j].frame = link, frame
        return arr

    def refused(h, rc, word, code=-1):
        assert rc == code, (rc, lib.pnr_last_error(h))
        assert word in lib.pnr_last_error(h), lib.pnr_last_error(h)

    good = specs((10, L.FRAME_WORLD), (3, L.FRAME_LINK))
    call = lib.pnr_get_joint_states
    assert call(None, None, None, None, 0, None, P(jo), P(ro), None) == -1
    kin = PioneerVectorEnv(n, device="cuda:0", seed=1)
    kin.reset()
    refused(kin._h, call(kin._h, None, None, None, 0, None, P(jo), P(ro), kin._stream()), b"dynamics mode", code=-5)
    kin.close()
    env = PioneerVectorEnv(n, device="cuda:0", seed=1, engine_config=EngineConfig(mode="dynamic"))
    refused(env._h, call(env._h, None, None, None, 0, None, P(jo), P(ro), env._stream()), b"before the first pnr_reset")
    env.close()
    env, _ = scenario("C", n)
    h, st = env._h, env._stream()
    before = (env.get_state().clone(), env.get_dyn_state().clone())
    refused(h, call(h, None, None, None, 0, None, None, P(ro), st), b"null joints_out")
    for args in ((P(js, 4), None, None, 0, None, P(jo), P(ro)), (None, P(tq, 4), None, 0, None, P(jo), P(ro)),
                 (None, None, good, 2, P(wr, 4), P(jo), P(ro)), (None, None, None, 0, None, P(jo, 4), P(ro)),
                 (None, None, None, 0, None, P(jo), P(ro, 4))):
        refused(h, call(h, *args, st), b"aligned")
    for k in (-1, 5, 1 << 20):
        refused(h, call(h, None, None, good, k, P(wr), P(jo), P(ro), st), b"n_specs")
    refused(h, call(h, None, None, None, 2, P(wr), P(jo), P(ro), st), b"null specs")
    refused(h, call(h, None, None, good, 2, None, P(jo), P(ro), st), b"null wrenches")
    refused(h, call(h, None, None, good, 0, None, P(jo), P(ro), st), b"n_specs 0")
    refused(h, call(h, None, None, None, 0, P(wr), P(jo), P(ro), st), b"n_specs 0")
    for link in (-1, 11, 1 << 20):
        refused(h, call(h, None, None, specs((10, L.FRAME_WORLD), (link, L.FRAME_LINK)), 2, P(wr), P(jo), P(ro), st), b"link")
    for frame in (0, 3, -1):
        refused(h, call(h, None, None, specs((10, frame)), 1, P(wr), P(jo), P(ro), st), b"frame")
    env.set_joint_motor(2, L.CONTROL_VELOCITY_CONSTRAINT, target_velocity=0.1)
    refused(h, call(h, None, P(tq), None, 0, None, P(jo), P(ro), st), b"constraint motor", code=-5)
    refused(h, call(h, None, None, good, 2, P(wr), P(jo), P(ro), st), b"constraint motor", code=-5)
    with pytest.raises(L.PnrError, match="constraint motor"):
        env.joint_states(joint_torques=tq[:n * 6].view(n, 6))
    with pytest.raises(AssertionError):
        env.joint_states(link_wrenches=([(10, "sideways")], wr[:n * 9].view(n, 1, 9)))
    torch.cuda.synchronize()
    assert bool((jo == SENTINEL).all()) and bool((ro == SENTINEL).all()), "a refused call touches no output"
    assert torch.equal(bits(env.get_state()), bits(before[0])) and torch.equal(bits(env.get_dyn_state()), bits(before[1]))
    assert call(h, None, None, None, 0, None, P(jo), None, st) == 0          # constraint motors alone, no reaction: accepted
    env.set_joint_motor(2, L.CONTROL_VELOCITY, target_velocity=0.0, velocity_gain=0.0, max_force=0.0)
    assert call(h, P(js), P(tq), good, 2, P(wr), P(jo), P(ro), st) == 0       # the PD law again: accepted
    torch.cuda.synchronize()
    assert bool((jo[:n * 24] != SENTINEL).all()) and bool((ro[:n * 36] != SENTINEL).all())
    assert bool((jo[n * 24:] == SENTINEL).all()) and bool((ro[n * 36:] == SENTINEL).all())
    env.close()


# ---- graph capture --------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_eager_result():
    n = 64
    env, I = scenario("C", n)
    wt, tq = dev(I["wrenches"]), dev(I["tau"])
    out = dict(joints=torch.zeros((n, 6, 4), device="cuda:0"), reaction=torch.zeros((n, 6, 6), device="cuda:0"))
    s = torch.cuda.Stream(device=env.device)
    s.wait_stream(torch.cuda.current_stream(env.device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        env.joint_states(joint_torques=tq, link_wrenches=(I["specs"], wt), out=out)     # warm-up on the capture stream
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            env.joint_states(joint_torques=tq, link_wrenches=(I["specs"], wt), out=out)
    torch.cuda.synchronize()
    eager = {k: v.clone() for k, v in out.items()}
    for v in out.values():
        v.fill_(SENTINEL)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(bits(out[k]), bits(eager[k])) for k in out)
    assert bool((out["joints"] != SENTINEL).all())
    env.close()


# ---- facade -----------------------------------------------------------------------------------------------------------------------------------
def test_facade_joint_state_sees_the_queued_shove_and_leaves_it_queued():
    from pioneer_amd import EngineConfig, PioneerKinematicEnv
    from pioneer_amd.scene import JointState

    def fresh():
        env = PioneerKinematicEnv(engine_config=EngineConfig(mode="dynamic"))
        env.reset_world(joint_positions=np.array([0.3, -0.4, 0.5, 0.2, -0.3, 0.1]), target_position=(20.0, 0.0, 4.0))
        for j in env.scene.joints:
            j.control_position(0.0, position_gain=0.0, velocity_gain=0.0)        # zero gains: no motor
        return env

    def qd(env):
        return np.array([j.velocity() for j in env.scene.joints])

    env, still = fresh(), fresh()
    J = env.scene.joints
    vec = env._vec.joint_states()
    st = J[2].state()
    assert isinstance(st, JointState) and st._fields == ("joint_position", "joint_velocity", "joint_reaction_forces", "applied_joint_motor_torque")
    assert st.joint_position == J[2].position() and st.joint_velocity == J[2].velocity()
    assert st.joint_reaction_forces == tuple(float(x) for x in vec["reaction"][0, 2]) and len(st.joint_reaction_forces) == 6
    assert st.applied_joint_motor_torque == float(vec["joints"][0, 2, 3]) == 0.0
    assert J[2].acceleration() == float(vec["joints"][0, 2, 2])
    assert [s.joint_position for s in env.scene.joint_states()] == [j.position() for j in J]
    rest = np.array(J[0].state().joint_reaction_forces)
    env.scene.links_by_name["robot:pointer"].apply_force((0.0, 50.0, 30.0))
    J[1].control_torque(3.0)
    pushed = np.array(J[0].state().joint_reaction_forces)
    print(f"facade: the queued force moves joint 0's reaction by {np.abs(pushed - rest).max():.3e}")
    assert np.abs(pushed - rest).max() > 1.0
    assert np.abs([j.acceleration() for j in J]).max() > 1.0
    assert len(env.world._wrenches) == 1 and env.world._torques == {1: 3.0}, "looked at, not consumed"
    env.world.step(); still.world.step()
    assert env.world._wrenches == [] and env.world._torques == {}
    assert np.abs(qd(env) - qd(still)).max() > 10 * QD_TOL, "the step still applied the shove"
    after = np.array(J[0].state().joint_reaction_forces)
    assert np.abs(after - pushed).max() > 1.0, "the next look carries no force"
    # kinematic mode: position and velocity as today, nothing simulated
    kin = PioneerKinematicEnv()
    kin.reset_world(joint_positions=np.array([0.3, -0.4, 0.5, 0.2, -0.3, 0.1]), target_position=(20.0, 0.0, 4.0))
    kin.scene.joints[3].reset_state(0.25, 0.5)
    ks = kin.scene.joints[3].state()
    assert ks == JointState(kin.scene.joints[3].position(), kin.scene.joints[3].velocity(), (0.0,) * 6, 0.0)
    assert (ks.joint_position, ks.joint_velocity) == (0.25, 0.5) and kin.scene.joints[3].acceleration() == 0.0
    kin.close(); still.close(); env.close()
