"""GPU tests of pnr_get_contacts (PioneerVectorEnv.contacts, Scene.contact_points / closest_points, evaluate()'s collision
figures) against the float64 reference of tests/contact_query_ref.py, on the inputs of tests/contact_query_cases.py.

Bars (cases.*): TIGHT = FLOOR_MARGIN (8) x what float32 arithmetic alone costs on these inputs, measured on the CPU in float32
numpy (tests/test_contact_query_cpu.py asserts the floors and that 8 x floor is inside the hard bars); HARD = the project's own:
distances, positions and normals 1e-4, forces kp 1e-4 + kd x the float32 velocity floor, torques that x the longest lever.  Both
are asserted.  A comparison leaves out only what contact_query_ref.exclusions names (two nearest bodies within 1e-3, a
box-interior face switch within 1e-3, for forces and torques |distance| < 1e-3); the CPU test asserts those are <= 1 % of the
pairs.  Every test prints its figures before it asserts.  MEASURED VALUES ON AN MI355X: see DESIGN.md 3j.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import contact_query_cases as cases
import contact_query_ref as ref
from bars import Q_TOL, QD_TOL
from gpu_support import dev, dyn_env, f64, kin_env, lib as _lib, load_joints

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
SIZES = list(cases.SIZES)
KEYS = ("points", "summary", "joint_torques")
# the facade scene's pose: arm1 leaning into the reference demo's box.  No pose inside the URDF limits puts a sample of arm1
# into that box (measured: none of 200 000 uniform poses; at the limit q2 = 1.309 arm1's last sample is still 0.15 clear of the
# box's top), so joint 2 sits at 1.467; reset_world takes its joint_positions as they are, like the reference's.
FACADE_POSE = (0.536, 1.467, -1.275, 0.446, -1.434, -1.607)


def scene_bodies(bodies=cases.SCENE_A):
    from pioneer_amd.config import scene_box, scene_plane, scene_sphere
    make = {"plane": lambda b: scene_plane(b["size"], b["position"], b["quat"]),
            "box": lambda b: scene_box(b["size"], b["position"], b["quat"]),
            "sphere": lambda b: scene_sphere(b["size"][0], b["position"])}
    return [make[b["shape"]](b) for b in bodies]


def make_kin(n, reset=True):
    return kin_env(n, cases.SEED, reset, auto_reset=False, max_episode_steps=0)


def make_dyn(n, gravity=9.81, frame_skip=1, **eng):
    return dyn_env(n, cases.SEED, gravity, frame_skip, **eng)


def source(kind, n, q, qd):
    """(env, joint_state argument) for a joint source holding q | qd"""
    if kind == "buffer":
        return make_kin(n), dev(np.concatenate([q, qd], axis=1))
    if kind == "dynamic_own":
        env = make_dyn(n)
        load_joints(env, q, qd)
        return env, None
    assert kind == "kinematic_own"                                    # the env's r (state words 12-17) and v (6-11)
    env = make_kin(n)
    w = env.get_state()
    f = w.view(torch.float32)
    f[6:12], f[12:18] = dev(qd.T), dev(q.T)
    env.set_state(w)
    return env, None


def check_against_reference(res, family, n):
    """every figure of one call against the reference's first n envs; prints, then asserts both bars"""
    r = cases.reference(family)
    ex = ref.exclusions(r)
    geo, frc = ~ex["geometry"][:n], ~ex["force"][:n]
    pts, want = f64(res["points"]), r["points"][:n]
    err = lambda sl, mask: float(np.abs(pts[..., sl] - want[..., sl])[mask].max())  # noqa: E731
    e_dist, e_nrm, e_pos, e_force = err(slice(0, 1), geo), err(slice(1, 4), geo), err(slice(4, 7), geo), err(slice(8, 9), frc)
    body_ok = bool(np.array_equal(pts[..., 7][geo], want[..., 7][geo]))
    sm, swant = f64(res["summary"]), r["summary"][:n]
    env_geo = geo.all(axis=1)
    e_sdist = float(np.abs(sm[:, 0] - swant[:, 0]).max())
    # samples 14 and 15 are one sphere (arm2's last sample and rotator2's first sit at the same point with the same radius:
    # contact_query_ref.TWIN_SAMPLES, asserted on the CPU), so which of the two carries the smallest distance is rounding
    idx_ok = bool(np.array_equal(ref.merge_twins(sm[env_geo, 1]), ref.merge_twins(swant[env_geo, 1]))
                  and np.array_equal(sm[env_geo, 2], swant[env_geo, 2]))
    count_env = (np.abs(want[..., 0]) >= 1e-4).all(axis=1)
    count_ok = bool(np.array_equal(sm[count_env, 3], swant[count_env, 3]))
    env_frc = frc.all(axis=1)
    e_tau = float(np.abs(f64(res["joint_torques"]) - r["torques"][:n])[env_frc].max()) if env_frc.any() else 0.0
    unit = float(np.abs(np.linalg.norm(pts[..., 1:4], axis=2) - 1.0).max())
    m = cases.FLOOR_MARGIN
    print(f"family {family} n={n}: distance {e_dist:.2e} (tight {m * cases.DIST_FLOOR:.1e}) normal {e_nrm:.2e} ({m * cases.NORMAL_FLOOR:.1e}) "
          f"position {e_pos:.2e} ({m * cases.POS_FLOOR:.1e}) force {e_force:.2e} ({m * cases.FORCE_FLOOR:.1e}) torque {e_tau:.2e} "
          f"({m * cases.TORQUE_FLOOR:.1e}) summary distance {e_sdist:.2e} | |n|-1 {unit:.1e} | penetrating pairs {(want[..., 0] < 0).mean():.3f} "
          f"| compared pairs {geo.mean():.4f} / {frc.mean():.4f}, envs {env_frc.mean():.3f}")
    assert geo.mean() >= 0.99 and frc.mean() >= 0.99 or n < 37
    assert body_ok and idx_ok and count_ok
    assert e_dist <= m * cases.DIST_FLOOR <= cases.DIST_HARD and e_sdist <= m * cases.DIST_FLOOR
    assert e_pos <= m * cases.POS_FLOOR <= cases.DIST_HARD
    assert e_nrm <= m * cases.NORMAL_FLOOR <= cases.NORMAL_HARD and unit <= cases.NORMAL_HARD
    assert e_force <= m * cases.FORCE_FLOOR <= cases.FORCE_HARD
    assert e_tau <= m * cases.TORQUE_FLOOR <= cases.TORQUE_HARD


# ---- 1. parity with the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["buffer", "dynamic_own", "kinematic_own"])
@pytest.mark.parametrize("n", SIZES)
def test_contacts_against_the_reference(n, kind):
    q, qd = cases.joints(n)
    env, js = source(kind, n, q, qd)
    before = None if js is None else js.clone()
    for family in "AB":
        bp = dev(cases.family_b_positions(n)) if family == "B" else None
        res = env.contacts(joint_state=js, bodies=scene_bodies(), body_positions=bp, joint_torques=True)
        torch.cuda.synchronize()
        check_against_reference(res, family, n)
    assert js is None or torch.equal(js, before)
    env.close()


# ---- 2. bounds and NULLs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_nothing_past_n_rows_and_each_output_alone(n):
    env = make_kin(n)
    js = dev(cases.joint_state(n))
    bp = dev(cases.family_b_positions(n))
    shapes = {"points": (ref.SAMPLES, ref.DIM), "summary": (4,), "joint_torques": (6,)}
    pad = 3
    big = {k: torch.full((n + pad,) + s, SENTINEL, device="cuda:0") for k, s in shapes.items()}
    out = {k: v[:n] for k, v in big.items()}
    res = env.contacts(joint_state=js, bodies=scene_bodies(), body_positions=bp, joint_torques=True, out=out)
    torch.cuda.synchronize()
    for k in KEYS:
        assert res[k].data_ptr() == big[k].data_ptr()
        assert bool((big[k][n:] == SENTINEL).all()), k               # nothing past row n
        assert not bool((big[k][:n] == SENTINEL).any()), k
    for k in KEYS:                                                    # each output alone: the same bits
        alone = env.contacts(joint_state=js, bodies=scene_bodies(), body_positions=bp, points=k == "points", summary=k == "summary",
                             joint_torques=k == "joint_torques")
        assert list(alone) == [k] and torch.equal(alone[k], res[k]), k
    none = env.contacts(joint_state=js, bodies=[], joint_torques=True)
    torch.cuda.synchronize()
    pts = none["points"]
    print(f"n={n}: no bodies -> distance {float(pts[0, 0, 0])}, body {float(pts[0, 0, 7])}, summary {none['summary'][0].tolist()}")
    assert bool(torch.isinf(pts[..., 0]).all()) and bool((pts[..., 0] > 0).all())
    assert bool((pts[..., 7] == -1).all()) and bool((pts[..., 8] == 0).all()) and bool((pts[..., 1:4] == 0).all())
    assert bool((none["joint_torques"] == 0).all())
    sm = none["summary"]
    assert bool(torch.isinf(sm[:, 0]).all()) and bool((sm[:, 1] == 0).all()) and bool((sm[:, 2] == -1).all()) and bool((sm[:, 3] == 0).all())
    # with bodies=None a body-less env asks about its own (empty) collision world
    assert torch.equal(env.contacts(joint_state=js)["points"], pts)
    env.close()


# ---- 3. batch independence ------------------------------------------------------------------------------------------------------
def test_an_envs_results_do_not_depend_on_the_batch():
    k, lane = 777, 5
    js_all, bp_all = cases.joint_state(cases.N_MAX), cases.family_b_positions(cases.N_MAX)
    big = make_kin(cases.N_MAX)
    in_batch = big.contacts(joint_state=dev(js_all), bodies=scene_bodies(), body_positions=dev(bp_all), joint_torques=True)
    one = make_kin(1)
    alone = one.contacts(joint_state=dev(js_all[k:k + 1]), bodies=scene_bodies(), body_positions=dev(bp_all[k:k + 1]), joint_torques=True)
    wave = make_kin(64)
    js64, bp64 = js_all[:64].copy(), bp_all[:64].copy()
    js64[lane], bp64[lane] = js_all[k], bp_all[k]
    moved = wave.contacts(joint_state=dev(js64), bodies=scene_bodies(), body_positions=dev(bp64), joint_torques=True)
    torch.cuda.synchronize()
    for key in KEYS:
        same = torch.equal(in_batch[key][k], alone[key][0]) and torch.equal(in_batch[key][k], moved[key][lane])
        print(f"{key}: env {k} alone / in a batch of {cases.N_MAX} / at lane {lane} of 64: {'bit-identical' if same else 'DIFFERENT'}")
        assert same
    assert float(in_batch["summary"][k, 3]) > 0 or float(in_batch["summary"][k, 0]) < 5      # the env is near something
    for e in (big, one, wave):
        e.close()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing():
    L = _lib()
    n = 64
    env = make_kin(n)
    lib, h, st = env.lib, env._h, env._stream()
    js = dev(cases.joint_state(n))
    bp = dev(cases.family_b_positions(n))
    pts = torch.full((n + 1, ref.SAMPLES, ref.DIM), SENTINEL, device="cuda:0")
    sm = torch.full((n + 1, 4), SENTINEL, device="cuda:0")
    tq = torch.full((n + 1, 6), SENTINEL, device="cuda:0")
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731

    def params(**kw):
        from pioneer_amd.config import fill_scene_body
        p = L.PnrContactParams()
        assert lib.pnr_contact_params_default(p) == 0
        bodies = scene_bodies()
        p.n_bodies = len(bodies)
        for i, b in enumerate(bodies):
            fill_scene_body(p.bodies[i], b, "body")
        for name, v in kw.items():
            setattr(p, name, v)
        return p

    def refused(what, hh, p, jsp, bpp, a, b, c):
        rc = lib.pnr_get_contacts(hh, jsp, p, bpp, a, b, c, st)
        msg = lib.pnr_last_error(hh).decode()
        torch.cuda.synchronize()
        print(f"{what!r}: rc {rc}, {msg!r}")
        assert rc == -1 and what in msg, (what, rc, msg)
        assert bool((pts == SENTINEL).all()) and bool((sm == SENTINEL).all()) and bool((tq == SENTINEL).all())

    ok = params()
    refused("null handle", None, ok, P(js), None, P(pts), P(sm), P(tq))
    refused("null params", h, None, P(js), None, P(pts), P(sm), P(tq))
    refused("struct_size", h, params(struct_size=8), P(js), None, P(pts), P(sm), P(tq))
    refused("n_bodies", h, params(n_bodies=-1), P(js), None, P(pts), P(sm), P(tq))
    refused("n_bodies", h, params(n_bodies=9), P(js), None, P(pts), P(sm), P(tq))
    bad = params(); bad.bodies[1].shape = 7
    refused("bad shape", h, bad, P(js), None, P(pts), P(sm), P(tq))
    bad = params(); bad.bodies[2].position[1] = float("nan")
    refused("non-finite data", h, bad, P(js), None, P(pts), P(sm), P(tq))
    bad = params(); bad.bodies[0].size[2] = float("inf")
    refused("non-finite data", h, bad, P(js), None, P(pts), P(sm), P(tq))
    bad = params()
    for i in range(4):
        bad.bodies[1].orientation[i] = 0.0
    refused("zero orientation quaternion", h, bad, P(js), None, P(pts), P(sm), P(tq))
    bad = params(); bad.bodies[1].size[0] = 0.0
    refused("box half extents", h, bad, P(js), None, P(pts), P(sm), P(tq))
    bad = params(); bad.bodies[2].size[0] = -1.0
    refused("sphere radius", h, bad, P(js), None, P(pts), P(sm), P(tq))
    bad = params()
    for i in range(3):
        bad.bodies[0].size[i] = 0.0
    refused("zero plane normal", h, bad, P(js), None, P(pts), P(sm), P(tq))
    refused("contact_kp and contact_kd", h, params(contact_kp=-1.0), P(js), None, P(pts), P(sm), P(tq))
    refused("contact_kp and contact_kd", h, params(contact_kd=float("nan")), P(js), None, P(pts), P(sm), P(tq))
    refused("contact_kp and contact_kd", h, params(contact_kp=float("inf")), P(js), None, P(pts), P(sm), P(tq))
    refused("16-byte aligned", h, ok, P(js), None, P(pts, 4), P(sm), P(tq))
    refused("16-byte aligned", h, ok, P(js), None, P(pts), P(sm, 8), P(tq))
    refused("16-byte aligned", h, ok, P(js), None, P(pts), P(sm), P(tq, 8))
    refused("16-byte aligned", h, ok, P(js, 4), None, P(pts), P(sm), P(tq))
    refused("4-byte aligned", h, ok, P(js), P(bp, 2), P(pts), P(sm), P(tq))
    refused("every output is NULL", h, ok, P(js), None, None, None, None)
    fresh = make_kin(n, reset=False)                                  # its own joints do not exist before the first reset
    refused("before the first pnr_reset", fresh._h, ok, None, None, P(pts), P(sm), P(tq))
    assert fresh.lib.pnr_get_contacts(fresh._h, P(js), ok, None, P(pts), None, None, st) == 0      # a caller's joints do
    torch.cuda.synchronize()
    assert not bool((pts[:n] == SENTINEL).any()) and bool((pts[n:] == SENTINEL).all())
    fresh.close()
    env.close()


# ---- 5. graph capture -----------------------------------------------------------------------------------------------------------
def test_the_call_is_captured_and_replayed():
    n = 1000
    env = make_kin(n)
    js_a, js_b = dev(cases.joint_state(n)), dev(cases.joint_state(n)[::-1].copy())
    bp = dev(cases.family_b_positions(n))
    js = js_a.clone()
    out = {"points": torch.empty((n, ref.SAMPLES, ref.DIM), device="cuda:0"), "summary": torch.empty((n, 4), device="cuda:0"),
           "joint_torques": torch.empty((n, 6), device="cuda:0")}
    call = lambda: env.contacts(joint_state=js, bodies=scene_bodies(), body_positions=bp, joint_torques=True, out=out)  # noqa: E731
    s = torch.cuda.Stream(device=env.device)
    s.wait_stream(torch.cuda.current_stream(env.device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        call()                                                        # warm-up on the capture stream
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):                           # a single chain: one kernel node
            call()
    torch.cuda.synchronize()
    for name, src in (("first replay", js_b), ("second replay", js_a)):
        js.copy_(src)
        for v in out.values():
            v.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        eager = env.contacts(joint_state=src, bodies=scene_bodies(), body_positions=bp, joint_torques=True)
        torch.cuda.synchronize()
        same = all(torch.equal(out[k], eager[k]) for k in KEYS)
        print(f"{name}: replayed outputs {'equal' if same else 'DIFFER from'} the eager call's bits")
        assert same
    env.close()


# ---- 6. the query is the step's contact model ---------------------------------------------------------------------------------------
def _step_poses(n):
    """n envs off their limits, half of them in SHALLOW contact (0.01 .. 0.3 deep, so that the contact forces stay of the order
    of the arm's weight and one float32 step stays comparable), half of them clear: chosen by the float64 reference from
    4 000 poses at 0.7 x the limits with |qd| <= 1"""
    lo, hi = cases.limits()
    q = np.random.default_rng(cases.SEED + 10).uniform(0.7 * lo, 0.7 * hi, size=(4000, 6)).astype(np.float32)
    qd = np.random.default_rng(cases.SEED + 11).uniform(-1.0, 1.0, size=(4000, 6)).astype(np.float32)
    d = ref.query(q, qd, cases.SCENE_A)["points"][:, :, 0].min(axis=1)
    touching = np.where((d < -0.01) & (d > -0.3))[0][:n // 2]
    clear = np.where(d > 0.5)[0][:n - len(touching)]
    assert len(touching) == n // 2 and len(clear) == n - n // 2
    pick = np.concatenate([touching, clear])
    return q[pick], qd[pick]


def test_query_torques_reproduce_a_step_with_contacts():
    L = _lib()
    n = 64
    q, qd = _step_poses(n)
    P = make_dyn(n, randomize=True, link_contacts=True, scene=tuple(scene_bodies()))
    Q = make_dyn(n, randomize=True, link_contacts=True)
    Q0 = make_dyn(n, randomize=True, link_contacts=True)
    d = P.get_dyn_state()
    d[0:6], d[6:12] = dev(q.T), dev(qd.T)
    for env in (P, Q, Q0):
        env.set_dyn_state(d.clone())
        for j in range(6):                                            # zero gains: no motor torque at all
            env.set_joint_motor(j, L.CONTROL_VELOCITY, target_velocity=0.0, velocity_gain=0.0, max_force=0.0)
    assert P.collision_bodies() == scene_bodies() and Q.collision_bodies() == []
    got = P.contacts(joint_torques=True)
    tau = got["joint_torques"]
    touching = int((got["summary"][:, 3] > 0).sum())
    P.world_step()
    Q.world_step(joint_torques=tau)
    Q0.world_step()
    torch.cuda.synchronize()
    p, qq, q0 = (f64(e.get_dyn_state()) for e in (P, Q, Q0))
    lo, hi = cases.limits()
    off_limits = bool((np.abs(p[0:6].T) < 0.95 * hi).all())
    eq, eqd = np.abs(p[0:6] - qq[0:6]).max(), np.abs(p[6:12] - qq[6:12]).max()
    without = np.abs(p[6:12] - q0[6:12]).max()
    print(f"{touching} of {n} envs in contact; |tau_c| up to {float(tau.abs().max()):.1f}; P against Q: |dq| {eq:.2e} (bar {Q_TOL:.0e}) "
          f"|dqd| {eqd:.2e} (bar {QD_TOL:.0e}); without the torques |dqd| {without:.2e}; off the limits {off_limits}")
    assert touching >= n // 4 and off_limits
    assert without > 10 * QD_TOL
    assert eq <= Q_TOL and eqd <= QD_TOL
    for env in (P, Q, Q0):
        env.close()


# ---- 7. the facade --------------------------------------------------------------------------------------------------------------
def test_facade_contact_points_in_pybullets_shape():
    from pioneer_amd import PioneerKinematicEnv
    from pioneer_amd.scene import ContactPoint
    env = PioneerKinematicEnv(device="cuda:0")
    quat = env.scene.rpy2quat((0, 0, 0))
    env.scene.create_body_box(name="obstacle:1", collision=True, mass=0.0, half_extents=(0.5, 0.5, 5.0), position=(10, 5, 0),
                              orientation=quat, rgba_color=(0, 0, 0, 1))
    env.scene.create_body_plane(name="ground", mass=0.0, normal=(0, 0, 1.0), position=(0, 0, 0), orientation=quat)
    env.reset_world(joint_positions=np.array(FACADE_POSE))
    cps = env.scene.contact_points()
    print(f"{len(cps)} contact points:", [(c.linkIndexA, c.bodyUniqueIdB, round(c.contactDistance, 3), round(c.normalForce, 1)) for c in cps])
    assert len(cps) >= 1 and all(isinstance(c, ContactPoint) for c in cps)
    assert ContactPoint._fields == ("contactFlag", "bodyUniqueIdA", "bodyUniqueIdB", "linkIndexA", "linkIndexB", "positionOnA",
                                    "positionOnB", "contactNormalOnB", "contactDistance", "normalForce")
    for c in cps:
        nrm, a, b = np.array(c.contactNormalOnB), np.array(c.positionOnA), np.array(c.positionOnB)
        assert c.contactDistance < 0 and c.normalForce >= 0 and c.linkIndexA == 3 and c.linkIndexB == -1
        assert c.bodyUniqueIdA == 0 and c.bodyUniqueIdB == 1                                   # the box was created first
        assert abs(np.linalg.norm(nrm) - 1.0) <= 1e-5
        assert np.abs((a - b) - c.contactDistance * nrm).max() <= 1e-5
        assert abs(c.normalForce - 2000.0 * -c.contactDistance) <= 1e-2                        # at rest: kp x depth
    near = env.scene.closest_points(1e9)
    assert len(near) == 23 and [c.linkIndexA for c in near] == list(ref.SAMPLE_LINKS)
    assert env.scene.contact_points(item=env.scene.links_by_name["robot:arm3"]) == []
    assert env.scene.contact_points(item=env.scene.links_by_name["robot:arm1"]) == cps
    assert env.scene.contact_points(item=env.scene.items_by_name["obstacle:1"]) == cps
    assert env.scene.contact_points(item=env.scene.items_by_name["ground"]) == []
    assert len(env.scene.closest_points(0.5)) < 23
    env.close()


def test_evaluate_reports_collisions_only_with_bodies(tmp_path):
    from pioneer_amd import EngineConfig, PioneerVectorEnv
    from pioneer_amd.evaluate import evaluate
    from pioneer_amd.ppo import PPOConfig, PPOTrainer
    env = PioneerVectorEnv(512, device="cuda:0", seed=1, engine_config=EngineConfig(max_episode_steps=20))
    tr = PPOTrainer(env, PPOConfig(rollout_fragment_length=8, num_sgd_iter=1, sgd_minibatch_size=2048))
    tr.train()
    ck = tr.save(str(tmp_path / "ck.pt"))
    env.close()
    box = EngineConfig(mode="dynamic", obstacle_position=(10.0, 5.0, 0.0), obstacle_half_extents=(0.5, 0.5, 5.0))
    with_box = evaluate(ck, episodes=1, max_episode_steps=4, engine_config=box)
    print({k: with_box[k] for k in ("collision_steps", "min_clearance", "episode_lengths")})
    assert 0.0 <= with_box["collision_steps"] <= 1.0 and np.isfinite(with_box["min_clearance"])
    bare = evaluate(ck, episodes=1, max_episode_steps=4)
    assert "collision_steps" not in bare and "min_clearance" not in bare
    assert set(with_box) - set(bare) == {"collision_steps", "min_clearance"}
